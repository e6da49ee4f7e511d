"""Evaluation of q-values against simulated truth (reference
hic3defdr/util/evaluation.py:15-100): the host functions, and beside them
the same on the GPU (``make_y_true_gpu``, ``roc_curve_gpu``,
``evaluate_gpu``; csrc/h3d_eval.hip), equal bit for bit."""
import numpy as np

from hic3defdr_amd.util.clusters import pixel_membership


def make_y_true(row, col, clusters, labels):
    """True for pixels inside a cluster whose label is not 'constit'
    (evaluation.py:15-41); vectorised pixel-key membership."""
    labels = np.asarray(labels)
    sig = [c for c, lab in zip(clusters, labels) if lab != 'constit']
    return pixel_membership(np.asarray(row), np.asarray(col), [sig])


def compute_fdr(y_true, y_pred):
    """fp / (fp + tp) (evaluation.py:82-100)."""
    y_true = np.asarray(y_true, dtype=bool)
    y_pred = np.asarray(y_pred, dtype=bool)
    fp = np.count_nonzero(y_pred & ~y_true)
    tp = np.count_nonzero(y_pred & y_true)
    return fp / float(fp + tp)


def evaluate(y_true, qvalues, n_fdr_points=100):
    """ROC (sklearn roc_curve on 1 - q, as the reference) plus the observed
    FDR at about ``n_fdr_points`` thresholds (evaluation.py:44-79). The FDR
    points are counted for all thresholds at once from one sort of the
    scores instead of a confusion matrix per threshold."""
    from sklearn.metrics import roc_curve
    y_true = np.asarray(y_true, dtype=bool)
    y_pred = 1 - np.asarray(qvalues)
    fpr, tpr, thresh = roc_curve(y_true, y_pred)
    if len(thresh) and np.isinf(thresh[0]):
        # scikit-learn >= 1.3 opens the curve at +inf; the reference's
        # scikit-learn (0.24, the version its outputs were produced with)
        # at the largest score + 1 -- kept, so eval.npz files compare
        thresh = thresh.copy()
        thresh[0] = thresh[1] + 1 if len(thresh) > 1 else 1.0
    fdr = np.ones_like(fpr) * np.nan
    rate = max(int(len(thresh) / n_fdr_points), 1)
    idx = np.arange(np.argmax(tpr > 0), len(thresh), rate)
    if idx.size:
        order = np.sort(y_pred)
        pos = np.sort(y_pred[y_true])
        # predicted positive at threshold t: y_pred >= t
        n_pred = len(order) - np.searchsorted(order, thresh[idx], side='left')
        tp = len(pos) - np.searchsorted(pos, thresh[idx], side='left')
        fdr[idx] = (n_pred - tp) / (n_pred).astype(float)
    return fdr, fpr, tpr, thresh


# ---- the same on the GPU (csrc/h3d_eval.hip) --------------------------------
# No CPU fallback: without libh3d.so or a gfx950 device these raise H3DError.
# Every argument is checked before anything is uploaded.

def make_y_true_gpu(row, col, clusters, labels):
    """``make_y_true`` with the membership test on the GPU
    (h3d_pixel_membership)."""
    from hic3defdr_amd.util.clusters import pixel_membership_gpu
    labels = np.atleast_1d(np.asarray(labels))
    if len(labels) != len(clusters):
        raise ValueError('%d labels for %d clusters'
                         % (len(labels), len(clusters)))
    sig = [c for c, lab in zip(clusters, labels) if lab != 'constit']
    return pixel_membership_gpu(row, col, [sig])


def _curve_args(y_true, y_score, what):
    y_true = np.asarray(y_true)
    if y_true.dtype.kind not in 'biu':
        raise TypeError('y_true must be boolean or integer, not %s'
                        % y_true.dtype)
    y_score = np.asarray(y_score)
    if y_score.dtype.kind not in 'fiu':
        raise TypeError('%s must be numeric, not %s' % (what, y_score.dtype))
    if y_true.ndim != 1 or y_score.ndim != 1:
        raise ValueError('y_true and %s must have 1 dimension' % what)
    if len(y_true) != len(y_score):
        raise ValueError('%d labels for %d %s'
                         % (len(y_true), len(y_score), what))
    if len(y_true) == 0:
        raise ValueError('no samples')
    if len(y_true) >= 2 ** 31:
        raise ValueError('at most 2^31 - 1 samples')
    y_score = np.ascontiguousarray(y_score, dtype=np.float64)
    if np.isnan(y_score).any():
        raise ValueError('%s contains NaN' % what)
    return np.ascontiguousarray(y_true.astype(bool)), y_score


def _curve(y_true, y_score, what, n_fdr_points, drop_intermediate,
           complement):
    import operator
    from hic3defdr_amd import _native
    n_fdr_points = operator.index(n_fdr_points)
    if n_fdr_points < 1:
        raise ValueError('n_fdr_points must be at least 1')
    y_true, y_score = _curve_args(y_true, y_score, what)
    res, flags = _native.context().roc_curve(
        y_true, y_score, n_fdr_points, drop_intermediate, complement)
    if flags:
        raise ValueError('%s contains NaN' % what)
    return res


def roc_curve_gpu(y_true, y_score, drop_intermediate=True):
    """``sklearn.metrics.roc_curve(y_true, y_score, drop_intermediate=...)``
    on the GPU (h3d_roc_curve): ``(fpr, tpr, thresh)``, equal to
    scikit-learn's except for the opening threshold, which is
    ``thresh[1] + 1`` (scikit-learn 0.24, see ``evaluate``). A NaN score and
    an empty input raise ValueError."""
    res = _curve(y_true, y_score, 'y_score', 100, drop_intermediate, False)
    return res['fpr'], res['tpr'], res['thresh']


def evaluate_gpu(y_true, qvalues, n_fdr_points=100):
    """``evaluate`` on the GPU: ``(fdr, fpr, tpr, thresh)``, equal to the
    host function's arrays bit for bit. The score ``1 - q`` is formed on the
    device; all four arrays come from one sort of (score, label)."""
    res = _curve(y_true, qvalues, 'qvalues', n_fdr_points, True, True)
    return res['fdr'], res['fpr'], res['tpr'], res['thresh']


def rates_at_threshold(eval_result, threshold=0.15):
    """``(fpr, fnr)`` at the point whose ``1 - thresh`` is closest to
    ``threshold`` (plotting/fn_vs_fp.py:63-68). ``eval_result``: a mapping
    with 'fpr', 'tpr' and 'thresh' (an ``eval.npz``) or the tuple
    ``(fdr, fpr, tpr, thresh)`` of ``evaluate``. Host code: the arrays are
    small."""
    if hasattr(eval_result, 'keys'):
        fpr, tpr, thresh = (np.asarray(eval_result[k])
                            for k in ('fpr', 'tpr', 'thresh'))
    else:
        _, fpr, tpr, thresh = (np.asarray(a) for a in eval_result)
    if not (fpr.ndim == 1 and fpr.shape == tpr.shape == thresh.shape):
        raise ValueError('fpr, tpr and thresh must be parallel vectors')
    if len(thresh) == 0:
        raise ValueError('an empty curve')
    idx = np.argmin(np.abs((1 - thresh) - threshold))
    return fpr[idx], (1 - tpr)[idx]
