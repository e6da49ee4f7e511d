"""Two bench.py --dump-outputs directories, array by array: shape, dtype and
raw bytes (NaNs compare by their bits).

    python tools/dump_compare.py <dir_a> <dir_b>

Exit status 1 when an array differs or is missing on one side.
"""
import os
import sys

import numpy as np


def main():
    a, b = sys.argv[1], sys.argv[2]
    names = sorted(set(os.listdir(a)) | set(os.listdir(b)))
    names = [n for n in names if n.endswith('.npy')]
    bad = 0
    for n in names:
        pa, pb = os.path.join(a, n), os.path.join(b, n)
        if not (os.path.exists(pa) and os.path.exists(pb)):
            print(n, 'MISSING on one side')
            bad += 1
            continue
        x, y = np.load(pa), np.load(pb)
        same = (x.shape == y.shape and x.dtype == y.dtype
                and x.tobytes() == y.tobytes())
        print(n, x.shape, 'EQUAL' if same else 'DIFFERENT')
        bad += 0 if same else 1
    print('dump compare: %d arrays, %d different' % (len(names), bad))
    return 1 if bad or not names else 0


if __name__ == '__main__':
    sys.exit(main())
