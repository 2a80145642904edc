"""TEST INFRASTRUCTURE: tests/mx_numpy_eval_reppoints.py (the evaluating numpy stand-in with the RepPoints operators)
extended by what RepPointsHead.get_prediction (models/RepPoints/builder.py:486-576) uses beyond it, so that the
method runs unmodified and produces numbers (tests/golden/make_golden_reppoints_decode.py).  Neither
mx_numpy_eval.py nor mx_numpy_eval_reppoints.py is edited.

Added, float32 throughout, as MXNet documents them:
  * `mx.symbol` is the namespace `mx.sym` (make_mx already binds both names to one module; asserted here);
  * `X.transpose(data, axes)`;
  * `X.sigmoid` is the IDENTITY: the fixture feeds probabilities, so that no libm enters the pinned bits (the same
    split as FCOS, whose CustomOps take probabilities); the device's fused sigmoid is pinned by a test of its own;
  * `topk` with k < 1 returns every element (MXNet: "k < 1 means all"); the order among equal keys stays the
    project's rule of mx_numpy_eval_reppoints._topk -- stable, the lower index first;
  * `max(axis=-1)`, `slice_axis` with a negative axis, `stack`, `split` (of im_info and of the boxes) and scalar
    arithmetic on arrays already work in the stand-ins this one extends; the fixture script exercises them.
"""
from . import mx_numpy_eval_reppoints as ER


def _topk(d, axis=-1, k=1, ret_typ="indices", is_ascend=False):
    return ER._topk(d, axis=axis, k=k if k >= 1 else d.v.shape[axis], ret_typ=ret_typ, is_ascend=is_ascend)


def extend(mx, X):
    """add the get_prediction operators to a stand-in made by mx_numpy_eval.make_mx(); returns the namespace `F`"""
    s = ER.extend(mx, X)
    assert mx.symbol is s
    s.topk = _topk
    X.transpose = lambda data, axes, name=None: ER.Arr(data.v.transpose(axes))
    X.sigmoid = lambda data, name=None: data
    return s
