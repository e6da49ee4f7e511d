"""Device code of libh3d.so in two source trees, kernel by kernel.

    python tools/device_code_compare.py PARENT_TREE HEAD_TREE [--names]
                                        [--jobs N] [--keep DIR]

For each tree: every hipcc unit of its hic3defdr_amd/build.py NATIVE_SRCS is
compiled with the flags build.py gives that unit (HIP_FLAGS, TU_FLAGS) plus
--offload-device-only -S. Every function of the listings -- the kernels (a
.amdhsa_kernel block) and the out-of-line device functions they call -- is
then compared between the trees OVER THE WHOLE LIBRARY BY DEMANGLED NAME (a
kernel may change units): its instruction text and, for a kernel, its
.amdhsa_ descriptor, after normalising what carries a function or module
counter (.LBB<k>_, BB<k>_ in loop comments, .Lfunc_end<k>, .Ltmp<k>,
.Lpost_getpc<k>) and the alignment of comments.

Prints per tree the copies and distinct names, the names in one tree only,
the names whose text or descriptor differ between the trees (apart: those
whose copies differ within the parent, the head holding some of them), and
the names compiled into more than one unit,
grouped by those units (--names lists them). Exit status 1 if a name is in
one tree only or differs.

A text comparison: it knows no instruction names.
"""
import argparse
import collections
import concurrent.futures
import importlib.util
import os
import re
import shutil
import subprocess
import sys
import tempfile

COUNTERS = [(re.compile(r'\.LBB\d+_'), '.LBB_'),
            (re.compile(r'\bBB\d+_'), 'BB_'),
            (re.compile(r'\.Lfunc_(begin|end)\d+'), r'.Lfunc_\1'),
            (re.compile(r'\.Ltmp\d+'), '.Ltmp'),
            (re.compile(r'\.Lpost_getpc\d+'), '.Lpost_getpc'),
            (re.compile(r'\s*;\s*'), ' ; ')]


def norm(line):
    line = line.strip()
    for pat, rep in COUNTERS:
        line = pat.sub(rep, line)
    return line.strip()


def load_build(tree):
    path = os.path.join(tree, 'hic3defdr_amd', 'build.py')
    spec = importlib.util.spec_from_file_location(
        'h3dbuild_' + re.sub(r'\W', '_', os.path.abspath(tree)), path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def listings(tree, outdir, jobs):
    """unit -> path of its device assembly listing"""
    b = load_build(tree)
    os.makedirs(outdir, exist_ok=True)
    cmds = {}
    for src, cc in b.NATIVE_SRCS:
        if cc != 'hipcc':
            continue
        out = os.path.join(outdir, src + '.s')
        cmds[src] = (out, [b.HIPCC] + b.HIP_FLAGS + b.TU_FLAGS.get(src, []) +
                     ['--offload-device-only', '-S', '-I', b.INC, '-o', out,
                      os.path.join(b.CSRC, src)])

    def run(item):
        src, (out, cmd) = item
        r = subprocess.run(cmd, stdout=subprocess.PIPE,
                           stderr=subprocess.PIPE, universal_newlines=True)
        if r.returncode:
            raise SystemExit('%s: %s\n%s' % (src, ' '.join(cmd), r.stderr))
        return src, out

    with concurrent.futures.ThreadPoolExecutor(jobs) as ex:
        return dict(ex.map(run, cmds.items()))


def functions(path):
    """mangled name -> (is_kernel, text lines, descriptor lines) of one
    listing; the descriptor holds the .amdhsa_ block and the function's
    resource symbols (.set <name>.num_vgpr, ...)"""
    funcs = {}
    typed = set()
    cur = None
    in_desc = False
    with open(path) as fh:
        for raw in fh:
            s = raw.strip()
            m = re.match(r'\.type\s+(\S+),@function', s)
            if m:
                typed.add(m.group(1))
                continue
            if cur is None:
                m = re.match(r'^([^\s:;]+):', raw)
                if m and m.group(1) in typed and m.group(1) not in funcs:
                    cur = m.group(1)
                    funcs[cur] = [False, [], []]
                    continue
                m = re.match(r'\.set\s+(\S+)\.(\w+),\s*(.*)', s)
                if m and m.group(1) in funcs:
                    funcs[m.group(1)][2].append(
                        '.set %s, %s' % (m.group(2), norm(m.group(3))))
                continue
            if s.startswith('.amdhsa_kernel'):
                funcs[cur][0] = in_desc = True
            elif s.startswith('.end_amdhsa_kernel'):
                in_desc = False
            elif in_desc:
                funcs[cur][2].append(norm(s))
            elif re.match(r'^\.Lfunc_end\d+:', raw):
                cur = None
            elif s and not s.startswith(('.section', '.p2align', '.text')):
                funcs[cur][1].append(norm(s))
    return funcs


def demangle(names):
    names = sorted(names)
    exe = shutil.which('llvm-cxxfilt') or shutil.which('c++filt')
    if not exe or not names:
        return {n: n for n in names}
    out = subprocess.run([exe], input='\n'.join(names) + '\n',
                         stdout=subprocess.PIPE, universal_newlines=True,
                         check=True).stdout.split('\n')
    return dict(zip(names, out))


class Tree:
    def __init__(self, tree, outdir, jobs):
        self.tree = tree
        per_unit = {u: functions(p)
                    for u, p in listings(tree, outdir, jobs).items()}
        dm = demangle({n for f in per_unit.values() for n in f})
        # demangled name -> [(unit, text, descriptor)], kernels and functions
        self.kernels = collections.defaultdict(list)
        self.devfuncs = collections.defaultdict(list)
        self.per_unit = {}
        for unit, funcs in sorted(per_unit.items()):
            self.per_unit[unit] = sum(1 for f in funcs.values() if f[0])
            for name, (is_kernel, text, desc) in funcs.items():
                (self.kernels if is_kernel else self.devfuncs)[dm[name]] \
                    .append((unit, tuple(text), tuple(desc)))


def versions(copies):
    return {(t, d) for _, t, d in copies}


def compare(kind, a, b, show_names):
    bad = 0
    for tag, t in (('parent', a), ('head', b)):
        total = sum(len(c) for c in t.values())
        print('%s, %s: %d copies under %d distinct names, %d redundant'
              % (kind, tag, total, len(t), total - len(t)))
    for tag, x, y in (('parent', a, b), ('head', b, a)):
        only = sorted(set(x) - set(y))
        print('%s only at the %s: %d' % (kind, tag, len(only)))
        for n in only:
            print('    %s  [%s]' % (n, ', '.join(u for u, _, _ in x[n])))
        bad += len(only)
    both = sorted(set(a) & set(b))
    same = some = 0
    for n in both:
        va, vb = versions(a[n]), versions(b[n])
        if len(va) == 1 and va == vb:
            same += 1
            continue
        if vb <= va:
            # the parent's own copies differ (the text of a function can
            # depend on what else its unit holds); the head has some of them
            some += 1
            print('    PARENT COPIES DIFFER, the head as in [%s], not as in '
                  '[%s]: %s' % (
                      ', '.join(u for u, t, d in a[n] if (t, d) in vb),
                      ', '.join(u for u, t, d in a[n] if (t, d) not in vb),
                      n))
            continue
        bad += 1
        what = []
        if {t for t, _ in va} != {t for t, _ in vb}:
            what.append('instruction text')
        if {d for _, d in va} != {d for _, d in vb}:
            what.append('descriptor')
        print('    DIFFERS (%s; %d parent / %d head versions): %s'
              % (', '.join(what), len(va), len(vb), n))
    print('%s in both: %d; instruction text and descriptor identical: %d; '
          'as some of the parent\'s differing copies: %d; different: %d'
          % (kind, len(both), same, some, len(both) - same - some))
    for tag, t in (('parent', a), ('head', b)):
        groups = collections.defaultdict(list)
        for n, copies in t.items():
            if len(copies) > 1:
                groups[tuple(sorted(u for u, _, _ in copies))].append(n)
        print('%s in more than one unit, %s: %d names, %d extra copies'
              % (kind, tag, sum(len(v) for v in groups.values()),
                 sum(len(v) * (len(k) - 1) for k, v in groups.items())))
        for units, names in sorted(groups.items()):
            print('    %4d  %s' % (len(names), ' + '.join(units)))
            if show_names:
                for n in sorted(names):
                    print('          %s' % n)
    return bad


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('parent')
    ap.add_argument('head')
    ap.add_argument('--names', action='store_true',
                    help='list the names compiled into more than one unit')
    ap.add_argument('--jobs', type=int, default=8)
    ap.add_argument('--keep', help='keep the listings under this directory')
    args = ap.parse_args()
    work = args.keep or tempfile.mkdtemp(prefix='h3d_devcmp_')
    try:
        a = Tree(args.parent, os.path.join(work, 'parent'), args.jobs)
        b = Tree(args.head, os.path.join(work, 'head'), args.jobs)
    finally:
        if not args.keep:
            shutil.rmtree(work, ignore_errors=True)
    for tag, t in (('parent', a), ('head', b)):
        print('kernels per unit, %s: %s' % (tag, ', '.join(
            '%s %d' % (u, k) for u, k in t.per_unit.items())))
    bad = compare('kernels', a.kernels, b.kernels, args.names)
    bad += compare('device functions', a.devfuncs, b.devfuncs, args.names)
    print('RESULT: %s' % ('identical' if not bad else
                          '%d names differ or are in one tree only' % bad))
    return 1 if bad else 0


if __name__ == '__main__':
    sys.exit(main())
