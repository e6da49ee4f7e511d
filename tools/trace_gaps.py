"""Idle gaps between kernels in a rocprofv3 --kernel-trace CSV, per bench
step (a step starts at the k_iota launch of estimate_disp's sort): kernel
busy time, span, and the gaps longer than a threshold with the kernels on
either side -- where the host holds the GPU up. With ``prep`` also the last
step's prep, k_iota to the first equalize launch (k_disp_work), kernel by
kernel with its hardware queue (and that first equalize launch as the last
row): start and end in us from the first key
kernel, the span of the prep and the time two of its kernels ran at once
(the two-stream prep, H3D_PREP_STREAMS=2).

    python tools/trace_gaps.py <kernel_trace.csv> [min_gap_us] [prep]
"""
import csv
import sys


def main():
    path = sys.argv[1]
    args = [a for a in sys.argv[2:] if a != 'prep']
    min_gap = float(args[0]) if args else 20.0
    queue = {}
    rows = []
    for r in csv.DictReader(open(path)):
        rows.append((int(r['Start_Timestamp']), int(r['End_Timestamp']),
                     r['Kernel_Name'].split('(')[0].split('<')[0][-40:]))
        queue[rows[-1]] = r.get('Queue_Id', '?')
    rows.sort(key=lambda t: t[0])
    steps, cur = [], []
    for r in rows:
        if r[2].endswith('k_iota') and cur:
            steps.append(cur)
            cur = []
        cur.append(r)
    steps.append(cur)
    for k, st in enumerate(steps[-4:]):
        busy = sum(e - s for s, e, _ in st) / 1e3
        span = (st[-1][1] - st[0][0]) / 1e3
        gaps = [((b[0] - a[1]) / 1e3, a[2], b[2]) for a, b in zip(st, st[1:])
                if (b[0] - a[1]) / 1e3 > min_gap]
        tot = sum(g for g, _, _ in gaps)
        print('step %d: %d kernels, busy %.3f ms, span %.3f ms, gaps > %g us: '
              '%.3f ms' % (k, len(st), busy / 1e3, span / 1e3, min_gap,
                           tot / 1e3))
        for g, a, b in gaps:
            print('   %8.1f us  %s -> %s' % (g, a, b))
    if 'prep' in sys.argv[2:]:
        prep(steps[-1], queue)


def prep(st, queue):
    """the prep of one step: k_iota .. the first k_disp_work"""
    end = next(i for i, r in enumerate(st) if 'k_disp_work' in r[2])
    ks = st[:end]
    t0 = next((r[0] for r in ks if 'k_dist_cond_keys' in r[2]), ks[0][0])
    print('prep of the last step, us from the first key kernel:')
    print('   %8s %8s %7s  %-5s %s' % ('start', 'end', 'us', 'queue', 'kernel'))
    for r in ks + [st[end]]:  # (the last row: the first equalize launch)
        print('   %8.1f %8.1f %7.1f  %-5s %s' % (
            (r[0] - t0) / 1e3, (r[1] - t0) / 1e3, (r[1] - r[0]) / 1e3,
            queue[r], r[2]))
    # time with two or more of the prep's kernels running
    ev = sorted([(r[0], 1) for r in ks] + [(r[1], -1) for r in ks])
    live, last, both = 0, 0, 0
    for t, d in ev:
        if live >= 2:
            both += t - last
        live, last = live + d, t
    print('prep span, first key kernel -> first k_disp_work: %.1f us; '
          'kernel time %.1f us; two kernels at once for %.1f us' % (
              (st[end][0] - t0) / 1e3, sum(r[1] - r[0] for r in ks) / 1e3,
              both / 1e3))


if __name__ == '__main__':
    main()
