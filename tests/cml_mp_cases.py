"""The exact CML fixture tests/golden/unit_cml_mp.npz (written by
tests/golden/make_golden_cml_mp.py) and the bounds the per-pixel NLL term and
the bounded dispersion search are held to against it: shared by
test_cml_mp_host.py (nll_pixel* through the host and self-test builds) and
test_gpu_cml_exact.py (k_brent, k_brent_gang and the multi-rank driver).

The bounds are derived; none is taken from what the code gives.

**Term.** |got - want| <= 32 eps S, with want the exact term sum_j lgamma(d_j
+ r) + lgamma(n r) - lgamma(z + n r) - n lgamma(r) (r = 1 / delta - 1 as
nll_const rounds it) and S = sum_j max(1, |lgamma(d_j + r)|) + max(1,
|lgamma(z + n r)|) + max(1, |lgamma(n r)|) + n max(1, |lgamma(r)|): each of
the 2 n + 2 log-gammas may be off by 32 eps of max(1, |its value|).
h3d_special.h claims 5e-15 absolute (22.5 eps) below 10 and ~1e-15 relative
(4.5 eps) above; the rest is room for the roundings of the row sum. Where want
is exactly 0 (all-zero pseudodata, n = 1) the same expression is an absolute
bound. (S is stored as a float32 rounded down: never a wider bound.)

**Segment.** With delta_got = disp / (1 + disp):

    lo - tol2 - 1e-8 <= delta_got <= hi + tol2 + 1e-8,

no failure flag, and delta_got inside [1e-4, 100/101].

- tol2(delta) = 2 (sqrt(2.2e-16) delta + 1e-5 / 3) is the search's own
  termination rule: scipy's bounded search (restated op for op by seg_step)
  stops when |xf - xm| <= tol2 - (b - a) / 2, xm the midpoint of its bracket
  [a, b]. Then xf - a = (xf - xm) + (b - a) / 2 <= tol2 and likewise b - xf:
  both ends of the bracket are within tol2 of xf. With exact comparisons the
  bracket of a unimodal objective holds its minimiser (every update keeps
  the best point inside and moves an end to a point that is no better), so
  |xf - delta_star| <= tol2, also where delta_star is an end of the interval.
- The comparisons are not exact: every objective value carries the
  evaluation noise E = sum_i 32 eps S_i + eps n_pixels sum_i |term_i| (the
  term bound per pixel, and the rounding of the segment sum: n_pixels
  additions, each within eps of a partial sum <= sum |term_i|). A comparison
  can only be flipped between points whose exact values differ by at most
  2 E, so the search behaves as an exact one whose minimiser may be any
  point of {delta : f(delta) <= f(delta_star) + 2 E} = [lo, hi] (stored
  from mp; the generator asserts hi - lo <= tol2 and unimodality).
- 1e-8 covers the pseudodata of the f = 1 runs through the whole qcml
  driver: with f = 1 the equalize pass returns the counts (the generator
  asserts oracle.equalize within 1e-9 relative; q2q's tested bar is 1e-10),
  and moving the data by 1e-6 relative moved the exact minimiser by 1e-7 at
  most, so 1e-8 has ~1000x margin and is 0.15 % of tol2.
"""
import numpy as np

from conftest import golden

EPS = 2.220446049250313e-16
TERM_UNITS = 32                     # eps of max(1, |lgamma|) per log-gamma
BRENT_A = 1e-4                      # kBrentA, kBrentB (csrc/h3d_model.h)
BRENT_B = 100. / (100 + 1)
PSEUDO_SLACK = 1e-8

TERM_N = (1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32)
TERM_FAMILIES = ('zeros', 'tiny', 'sparse', 'frac', 'benign', 'large',
                 'mixed')
NPIX = 32
SEG_N = (2, 3, 4, 5, 8, 9, 16, 17, 32)
SEG_FAMILIES = ('benign', 'over', 'huge', 'poisson', 'under', 'ceiling',
                'sparse', 'large', 'frac')
SEG_LEN = 65
SEG_LONG = tuple((fam, n, ln) for fam in ('benign', 'sparse')
                 for n in (2, 4) for ln in (1025, 2049))
# the families of the f = 1 runs through the whole qcml driver: integer
# counts, no all-zero pixel. Left out:
# - huge and ceiling: at delta near 0.97 a tol2 move in delta is more than
#   qcml's 1e-4 in disp, and the loop may not settle;
# - over: qcml starts at disp = 0.01, where a count drawn at dispersion 2
#   (2032 at a fitted mean of ~380) lies beyond the double range of the NB
#   tail and q2q returns inf, in the reference as here. Its NLL is NaN, the
#   bounded search fails and the reference's ``assert res.success`` fires
#   (oracle.qcml raises on over at n = 8 .. 32; kFlagBrentFail here). There
#   is no result to hold to the bound. The general form (r < 5) is reached
#   through sparse, whose optimum is at r ~ 0.5.
QCML_FAMILIES = ('benign', 'poisson', 'under', 'sparse', 'large')
# h3dt_nll_terms' forms: general, mid, large, r >= 5, n r >= 5 (in_domain)
MODES = (0, 1, 2, 3, 4)


def tol2(delta):
    return 2.0 * (np.sqrt(2.2e-16) * np.abs(delta) + 1e-5 / 3.0)


def r_of(delta):
    """nll_const's arithmetic"""
    return 1. / delta - 1


def delta_for(r):
    """a delta whose r = 1 / delta - 1 is >= r by as little as the rounding
    allows (test_gpu_nll_ranges._delta_for)"""
    delta = 1. / (1. + r)
    while 1. / delta - 1 < r:
        delta = np.nextafter(delta, 0.)
    return delta


def term_deltas():
    """the ends of the search interval, both sides of the form switches at
    r = 5, 10, 20 (one representable delta either side), and four interior
    points"""
    out = [BRENT_A, BRENT_B]
    for r in (5., 10., 20.):
        # the largest delta whose r is still >= the switch, its neighbour
        # above (r below the switch) and the first delta below it whose r
        # is another double (two neighbouring deltas may round to one r)
        d = delta_for(r)
        while r_of(np.nextafter(d, 1.)) >= r:
            d = np.nextafter(d, 1.)
        up = np.nextafter(d, 0.)
        while r_of(up) == r_of(d):
            up = np.nextafter(up, 0.)
        out += [np.nextafter(d, 1.), d, up]
    out += [0.01, 0.3, 0.6, 0.9]
    return np.array(out, dtype=np.float64)


def in_domain(mode, delta, n):
    r = r_of(delta)
    nr = n * r
    if mode == 0:
        return True
    if mode == 1:
        return r >= 10.
    if mode == 2:
        return r >= 20.
    if mode == 3:
        return r >= 5. and nr >= 10. and n >= 2
    if mode == 4:
        return nr >= 5. and n >= 2
    raise ValueError(mode)


def seg_key(family, n, length=SEG_LEN):
    return 'seg_%s_n%d_L%d' % (family, n, length)


def seg_cases():
    """(family, n, length) of every segment case, in fixture order"""
    out = [(fam, n, SEG_LEN) for fam in SEG_FAMILIES for n in SEG_N]
    return out + list(SEG_LONG)


_cache = {}


def fixture():
    if 'g' not in _cache:
        _cache['g'] = golden('unit_cml_mp.npz')
    return _cache['g']


class Segment:
    def __init__(self, family, n, length=SEG_LEN):
        g = fixture()
        key = seg_key(family, n, length)
        if key + '_data' not in g:
            raise KeyError('%s is not in the fixture (dropped: %s)'
                           % (key, g['seg_dropped']))
        self.family, self.n, self.length, self.key = family, n, length, key
        self.data = np.ascontiguousarray(g[key + '_data'], dtype=np.float64)
        assert self.data.shape == (length, n)
        (self.delta_star, self.E, self.lo, self.hi, self.oracle,
         self.f1_err) = (float(v) for v in g[key + '_ref'])

    def bounds(self, delta):
        """the interval delta must lie in (tol2 at the search's own final
        point, as its termination rule takes it)"""
        t = tol2(delta) if np.isfinite(delta) else tol2(self.delta_star)
        return self.lo - t - PSEUDO_SLACK, self.hi + t + PSEUDO_SLACK


def segment(family, n, length=SEG_LEN):
    key = seg_key(family, n, length)
    if key not in _cache:
        _cache[key] = Segment(family, n, length)
    return _cache[key]


def have_segment(family, n, length=SEG_LEN):
    return seg_key(family, n, length) + '_data' in fixture()


def check_segment(seg, disp, flag, what):
    """Print the distance to delta_star as a fraction of the bound, then
    assert the segment bound. Returns that fraction."""
    disp = float(disp)
    delta = disp / (1. + disp)
    lo, hi = seg.bounds(delta)
    # the bound's reach on the side delta lies on
    reach = (hi - seg.delta_star) if delta >= seg.delta_star \
        else (seg.delta_star - lo)
    frac = abs(delta - seg.delta_star) / reach
    print('%s %-8s n=%-2d L=%-4d delta=%.12g delta_star=%.12g [%.12g, %.12g] '
          'flag=%d fraction_of_bound=%.3f'
          % (what, seg.family, seg.n, seg.length, delta, seg.delta_star, lo,
             hi, flag, frac))
    assert flag == 0, (what, seg.key, flag)
    assert np.isfinite(disp), (what, seg.key, disp)
    assert BRENT_A <= delta <= BRENT_B, (what, seg.key, delta)
    assert lo <= delta <= hi, (what, seg.key, delta, lo, hi)
    return frac


def term_cases(n):
    """(data (7, 32, n), want (7, 15, 32), S (7, 15, 32)) of one replicate
    count"""
    g = fixture()
    return (np.ascontiguousarray(g['term_n%d_data' % n]),
            g['term_n%d_want' % n],
            g['term_n%d_S' % n].astype(np.float64))


def term_units(got, want, S):
    """the error in units of the term bound (<= 1 passes)"""
    return np.abs(np.asarray(got) - want) / (TERM_UNITS * EPS * S)
