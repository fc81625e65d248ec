"""An eager ``tensorflow`` stand-in for the golden maker make_model_wiring_golden.py -- BUILD CONTAINER ONLY, no test imports it.

The reference's model code (backbones/ARU_v1.py, gnn/model/graph_util/layers.py, gnn/model/graph/graph_gnn.py, message_fn_chunk.py,
update_fn_lstm.py, the edge correction of graph_util/misc.py) is TensorFlow 1.x graph-definition Python.  TensorFlow does not exist
here; this module is put into ``sys.modules`` as ``tensorflow`` so that the reference's OWN code runs, op by op, on numpy arrays in
float64.  What that pins: which layer follows which, which scope name every variable gets and which variables are shared, the
concat / split / gate orders, the chunking of the message function -- all decided by the reference's code executing.

What it does NOT pin: the semantics of the ops themselves.  SAME padding, the crop of a transposed convolution, the divisor of an
average pool at the border, tf.sparse.softmax / reduce_max over stored entries, tf.sets.difference's sorted result ... are restated
HERE from the TensorFlow 1.x documentation -- a third writing, independent of oracle/ and of the product (neither is imported), but a
restatement all the same.  The frozen nets and TensorFlow's kernels stay unpinned.

Only the API those files touch when they run is implemented.  Everything else raises: an unknown attribute of the module, an
unknown keyword, an unknown submodule import.  Nothing returns a placeholder.

  install()                     -> puts the modules into sys.modules (before any ``import tensorflow`` of the reference)
  VARIABLES.reset(source)       -> new variable store; ``source(name, shape)`` supplies every value on creation
  VARIABLES.created             -> OrderedDict name -> value in creation order
  self_check()                  -> a handful of op checks against torch-CPU, run by the maker before it generates
"""
import contextlib
import importlib.abc
import sys
import types
from collections import OrderedDict

import numpy as np


# ---------------------------------------------------------------------------------------------------------------------------
# tensors
# ---------------------------------------------------------------------------------------------------------------------------
class DType:
    def __init__(self, name, kind):
        self.name, self.kind = name, kind

    def __repr__(self):
        return f"tf.{self.name}"


float32, float64 = DType("float32", "f"), DType("float64", "f")
int32, int64 = DType("int32", "i"), DType("int64", "i")
bool_ = DType("bool", "b")


class TensorShape(tuple):
    def as_list(self):
        return list(self)


def _raw(x):
    """python / numpy / Tensor -> numpy"""
    if isinstance(x, Tensor):
        return x._v
    if isinstance(x, (list, tuple)):
        return np.asarray([_raw(v) for v in x])
    if isinstance(x, SparseTensor):
        raise TypeError("a SparseTensor where a dense tensor is needed")
    return np.asarray(x)


def _ints(shape):
    """a shape / begin / size argument: int, Tensor or a list of them -> tuple of python ints"""
    a = _raw(shape)
    if a.dtype.kind not in "iu":
        if a.dtype.kind == "f" and np.all(a == np.round(a)):       # TF accepts 8.0 where a dimension is meant (Dimension(8.0) == 8)
            a = a.astype(np.int64)
        else:
            raise TypeError(f"not an integer shape: {shape!r}")
    return tuple(int(v) for v in np.atleast_1d(a))


class Tensor:
    __array_priority__ = 1000

    def __init__(self, value):
        v = np.asarray(_raw(value))
        if v.dtype.kind == "f":
            v = v.astype(np.float64)
        elif v.dtype.kind in "iu":
            v = v.astype(np.int64)
        elif v.dtype.kind != "b":
            raise TypeError(f"unsupported dtype {v.dtype}")
        self._v = v

    # -- shape -----------------------------------------------------------------------------------------------------------
    @property
    def shape(self):
        return TensorShape(self._v.shape)

    def get_shape(self):
        return self.shape

    def set_shape(self, shape):
        shape = list(shape)
        if len(shape) != self._v.ndim or any(s is not None and int(s) != d for s, d in zip(shape, self._v.shape)):
            raise ValueError(f"set_shape({shape}) on a tensor of shape {self._v.shape}")

    @property
    def dtype(self):
        return {"f": float32, "i": int32, "b": bool_}[self._v.dtype.kind]

    def numpy(self):
        return self._v

    def __repr__(self):
        return f"<standin Tensor {self._v.shape} {self._v.dtype}>"

    def __len__(self):
        return len(self._v)

    def _scalar(self, kinds):
        if self._v.ndim != 0 or self._v.dtype.kind not in kinds:
            raise TypeError(f"{self!r} is not a scalar of kind {kinds}")
        return self._v.item()

    def __int__(self):
        return int(self._scalar("i"))

    __index__ = __int__

    def __float__(self):
        return float(self._scalar("fi"))

    def __bool__(self):
        return bool(self._scalar("b"))

    __hash__ = object.__hash__                                   # (== stays identity, as for a TF1 tensor)

    def __getitem__(self, key):
        def conv(k):
            if isinstance(k, Tensor):
                return int(k) if k._v.ndim == 0 else k._v
            if isinstance(k, slice):
                return slice(*(None if p is None else int(p) for p in (k.start, k.stop, k.step)))
            return k
        key = tuple(conv(k) for k in key) if isinstance(key, tuple) else conv(key)
        return Tensor(self._v[key])

    # -- arithmetic --------------------------------------------------------------------------------------------------------
    def _bin(self, other, fn, swap=False):
        a, b = self._v, _raw(other)
        return Tensor(fn(b, a) if swap else fn(a, b))

    def __add__(self, o): return self._bin(o, np.add)
    def __radd__(self, o): return self._bin(o, np.add, True)
    def __sub__(self, o): return self._bin(o, np.subtract)
    def __rsub__(self, o): return self._bin(o, np.subtract, True)
    def __mul__(self, o): return self._bin(o, np.multiply)
    def __rmul__(self, o): return self._bin(o, np.multiply, True)
    def __truediv__(self, o): return self._bin(o, np.true_divide)
    def __rtruediv__(self, o): return self._bin(o, np.true_divide, True)
    def __floordiv__(self, o): return self._bin(o, np.floor_divide)
    def __rfloordiv__(self, o): return self._bin(o, np.floor_divide, True)
    def __mod__(self, o): return self._bin(o, np.mod)
    def __pow__(self, o): return self._bin(o, np.power)
    def __rpow__(self, o): return self._bin(o, np.power, True)
    def __neg__(self): return Tensor(-self._v)
    def __lt__(self, o): return self._bin(o, np.less)
    def __le__(self, o): return self._bin(o, np.less_equal)
    def __gt__(self, o): return self._bin(o, np.greater)
    def __ge__(self, o): return self._bin(o, np.greater_equal)


class SparseTensor:
    def __init__(self, indices, values, dense_shape):
        self.indices = Tensor(indices)
        self.values = Tensor(values)
        self.dense_shape = _ints(dense_shape)
        idx = self.indices._v
        if idx.ndim != 2 or idx.shape[1] != len(self.dense_shape) or idx.shape[0] != self.values._v.shape[0]:
            raise ValueError("SparseTensor: indices / values / dense_shape do not fit")
        if idx.size and (idx.min() < 0 or np.any(idx >= np.asarray(self.dense_shape))):
            raise ValueError("SparseTensor: index out of range")


def _canonical(indices):
    """row-major (lexicographic) order of sparse indices, stable"""
    return np.lexsort(tuple(indices[:, k] for k in range(indices.shape[1] - 1, -1, -1)))


def _need2d(sp, what):
    if not isinstance(sp, SparseTensor) or len(sp.dense_shape) != 2:
        raise NotImplementedError(f"{what}: a rank-2 SparseTensor is needed")
    idx = sp.indices._v
    if len({(int(a), int(b)) for a, b in idx}) != idx.shape[0]:
        raise NotImplementedError(f"{what}: duplicate indices")


def _sparse_reorder(sp):
    order = _canonical(sp.indices._v)
    return SparseTensor(sp.indices._v[order], sp.values._v[order], sp.dense_shape)


def _sparse_transpose(sp, perm=None):
    n = len(sp.dense_shape)
    perm = list(range(n - 1, -1, -1)) if perm is None else list(perm)
    idx = sp.indices._v[:, perm]
    return _sparse_reorder(SparseTensor(idx, sp.values._v, [sp.dense_shape[p] for p in perm]))      # the result is canonically ordered


def _sparse_softmax(sp):
    """over the last axis, the stored entries of a row only"""
    _need2d(sp, "sparse.softmax")
    idx, val = sp.indices._v, sp.values._v.astype(np.float64)
    out = np.empty_like(val)
    for r in np.unique(idx[:, 0]):
        m = idx[:, 0] == r
        e = np.exp(val[m] - val[m].max())
        out[m] = e / e.sum()
    return SparseTensor(idx, out, sp.dense_shape)


def _sparse_reduce(sp, axis, how):
    _need2d(sp, f"sparse.reduce_{how}")
    if axis not in (0, 1, -1, -2):
        raise NotImplementedError(f"sparse.reduce_{how}: axis {axis!r}")
    keep = 1 if axis in (0, -2) else 0
    idx, val = sp.indices._v, sp.values._v
    out = np.zeros(sp.dense_shape[keep], val.dtype)
    if how == "sum":
        np.add.at(out, idx[:, keep], val)
    else:                                                   # the implicit zeros take no part; a slice without entries reduces to 0
        for j in np.unique(idx[:, keep]):
            out[j] = val[idx[:, keep] == j].max()
    return Tensor(out)


def _sets_difference(a, b):
    a, b = _raw(a), _raw(b)
    if a.ndim != 2 or b.ndim != 2 or a.shape[0] != 1 or b.shape[0] != 1:
        raise NotImplementedError("sets.difference: [1, n] operands only")
    vals = np.setdiff1d(a[0], b[0])                         # sorted ascending, unique
    idx = np.stack([np.zeros(len(vals), np.int64), np.arange(len(vals), dtype=np.int64)], axis=1)
    return SparseTensor(idx, vals, [1, max(len(vals), 1)])


# ---------------------------------------------------------------------------------------------------------------------------
# variables and scopes
# ---------------------------------------------------------------------------------------------------------------------------
class _AutoReuse:
    def __repr__(self):
        return "AUTO_REUSE"


AUTO_REUSE = _AutoReuse()


class VariableScope:
    def __init__(self, name, reuse):
        self.name, self.reuse = name, reuse

    def reuse_variables(self):
        self.reuse = True


class _VariableStore:
    def __init__(self):
        self.reset(None)

    def reset(self, source):
        self.source = source
        self.created = OrderedDict()
        self.scopes = [VariableScope("", None)]


VARIABLES = _VariableStore()


@contextlib.contextmanager
def variable_scope(name_or_scope, default_name=None, values=None, reuse=None):
    if not isinstance(name_or_scope, str) or not name_or_scope:
        raise NotImplementedError(f"variable_scope({name_or_scope!r}): only a non-empty name")
    parent = VARIABLES.scopes[-1]
    scope = VariableScope(parent.name + "/" + name_or_scope if parent.name else name_or_scope,
                          parent.reuse if reuse in (None, False) else reuse)        # None / False inherit (TF 1.x)
    VARIABLES.scopes.append(scope)
    try:
        yield scope
    finally:
        VARIABLES.scopes.pop()


def get_variable_scope():
    return VARIABLES.scopes[-1]


def get_variable(name, shape=None, dtype=None, initializer=None):
    if VARIABLES.source is None:
        raise RuntimeError("VARIABLES.reset(source) first")
    scope = VARIABLES.scopes[-1]
    full = scope.name + "/" + name if scope.name else name
    shp = _ints(shape)
    if full in VARIABLES.created:
        if scope.reuse is not True and scope.reuse is not AUTO_REUSE:
            raise ValueError(f"Variable {full} already exists, disallowed. Did you mean to set reuse=True or reuse=tf.AUTO_REUSE in VarScope?")
        if VARIABLES.created[full].shape != shp:
            raise ValueError(f"Trying to share variable {full}, but specified shape {shp} and found shape {VARIABLES.created[full].shape}.")
        return Tensor(VARIABLES.created[full])
    if scope.reuse is True:
        raise ValueError(f"Variable {full} does not exist, or was not created with tf.get_variable().")
    if not isinstance(initializer, _Initializer):
        raise NotImplementedError(f"get_variable({full}): initializer {initializer!r}")
    value = np.asarray(VARIABLES.source(full, shp))
    if value.shape != shp:
        raise ValueError(f"the variable source returned shape {value.shape} for {full} {shp}")
    VARIABLES.created[full] = value
    return Tensor(value)


class _Initializer:
    """never evaluated: every value comes from the maker's source"""
    def __init__(self, *a, **k):
        pass


@contextlib.contextmanager
def name_scope(name, default_name=None, values=None):
    yield (name or default_name or "") + "/"


# ---------------------------------------------------------------------------------------------------------------------------
# dense ops
# ---------------------------------------------------------------------------------------------------------------------------
def _np_dtype(dtype, default):
    if dtype is None:
        return default
    if not isinstance(dtype, DType):
        raise TypeError(f"dtype {dtype!r}")
    return {"f": np.float64, "i": np.int64, "b": np.bool_}[dtype.kind]


def shape(x, name=None):
    return Tensor(np.asarray(_raw(x).shape, np.int64))


def constant(value, dtype=None, shape=None, name="Const"):
    v = np.asarray(_raw(value))
    v = v.astype(_np_dtype(dtype, v.dtype))
    if shape is not None:
        shp = _ints(shape)
        v = np.full(shp, v.item()) if v.ndim == 0 else v.reshape(shp)
    return Tensor(v)


def convert_to_tensor(value, dtype=None, name=None):
    return Tensor(_raw(value).astype(_np_dtype(dtype, _raw(value).dtype)))


def identity(x, name=None):
    return Tensor(_raw(x))


def Print(input_, data, message=None, first_n=None, summarize=None, name=None):
    return Tensor(_raw(input_))


def cast(x, dtype, name=None):
    v = _raw(x)
    if dtype.kind == "i" and v.dtype.kind == "f":
        v = np.trunc(v)
    return Tensor(v.astype(_np_dtype(dtype, None)))


def zeros(shape, dtype=float32, name=None):
    return Tensor(np.zeros(_ints(shape), _np_dtype(dtype, None)))


def ones(shape, dtype=float32, name=None):
    return Tensor(np.ones(_ints(shape), _np_dtype(dtype, None)))


def range_(start, limit=None, delta=1, dtype=None, name="range"):
    if limit is None:
        start, limit = 0, start
    return Tensor(np.arange(int(Tensor(start)), int(Tensor(limit)), int(Tensor(delta)), dtype=np.int64))


def stack(values, axis=0, name="stack"):
    return Tensor(np.stack([_raw(v) for v in values], axis=axis))


def unstack(value, num=None, axis=0, name="unstack"):
    v = _raw(value)
    return [Tensor(np.take(v, i, axis=axis)) for i in range(v.shape[axis])]


def concat(values, axis, name="concat"):
    vals = [_raw(v) for v in values]
    kinds = {v.dtype.kind for v in vals}
    if len(kinds) != 1:
        raise TypeError(f"concat of mixed dtypes {[v.dtype for v in vals]}")
    nd = {v.ndim for v in vals}
    if len(nd) != 1:
        raise ValueError("concat of tensors of different rank")
    return Tensor(np.concatenate(vals, axis=int(axis)))


def split(value, num_or_size_splits, axis=0, num=None, name="split"):
    v = _raw(value)
    if not isinstance(num_or_size_splits, int) or v.shape[axis] % num_or_size_splits:
        raise NotImplementedError("split: an integer number of equal parts only")
    return [Tensor(p) for p in np.split(v, num_or_size_splits, axis=axis)]


def add_n(inputs, name=None):
    vals = [_raw(v) for v in inputs]
    if len({v.shape for v in vals}) != 1:
        raise ValueError("add_n: shapes differ")
    out = vals[0].copy()
    for v in vals[1:]:
        out = out + v
    return Tensor(out)


def reshape(tensor, shape, name=None):
    return Tensor(_raw(tensor).reshape(_ints(shape)))


def transpose(a, perm=None, name="transpose"):
    return Tensor(np.transpose(_raw(a), None if perm is None else _ints(perm)))


def expand_dims(input, axis=None, name=None):
    return Tensor(np.expand_dims(_raw(input), int(axis)))


def squeeze(input, axis=None, name=None):
    return Tensor(np.squeeze(_raw(input), axis=axis))


def tile(input, multiples, name=None):
    return Tensor(np.tile(_raw(input), _ints(multiples)))


def reverse(tensor, axis, name=None):
    return Tensor(np.flip(_raw(tensor), axis=tuple(_ints(axis))))


def slice_(input_, begin, size, name=None):
    v = _raw(input_)
    begin, size = _ints(begin), _ints(size)
    if len(begin) != v.ndim or len(size) != v.ndim:
        raise ValueError("slice: begin / size rank")
    sl = []
    for b, s, d in zip(begin, size, v.shape):
        e = d if s == -1 else b + s
        if b < 0 or e > d:
            raise ValueError(f"slice [{b}, {e}) out of a dimension of {d}")
        sl.append(slice(b, e))
    return Tensor(v[tuple(sl)])


def gather(params, indices, validate_indices=None, name=None, axis=0):
    p, i = _raw(params), _raw(indices)
    if i.size and (i.min() < 0 or i.max() >= p.shape[axis]):
        raise IndexError("gather: index out of range")
    return Tensor(np.take(p, i, axis=axis))


def gather_nd(params, indices, name=None):
    p, i = _raw(params), _raw(indices)
    k = i.shape[-1]
    if k > p.ndim:
        raise ValueError("gather_nd: index depth")
    for d in range(k):
        if i.size and (i[..., d].min() < 0 or i[..., d].max() >= p.shape[d]):
            raise IndexError("gather_nd: index out of range")
    return Tensor(p[tuple(i[..., d] for d in range(k))])


def where(condition, x=None, y=None, name=None):
    if x is not None or y is not None:
        raise NotImplementedError("where(condition, x, y)")
    return Tensor(np.argwhere(_raw(condition)).astype(np.int64))


def sequence_mask(lengths, maxlen=None, dtype=bool_, name=None):
    ln = _raw(lengths)
    m = int(ln.max()) if maxlen is None else int(Tensor(maxlen))
    return Tensor((np.arange(m)[None, :] < ln[..., None]).astype(_np_dtype(dtype, None)))


def unique(x, out_idx=int32, name=None):
    v = _raw(x)
    if v.ndim != 1:
        raise ValueError("unique: 1-D only")
    vals, first, inv = np.unique(v, return_index=True, return_inverse=True)
    order = np.argsort(first, kind="stable")                # TF keeps the order of first occurrence
    rank = np.empty_like(order)
    rank[order] = np.arange(len(order))
    return Tensor(vals[order]), Tensor(rank[inv])


def _reduce(fn):
    def op(input_tensor, axis=None, keepdims=False, name=None):
        ax = None if axis is None else (tuple(_ints(axis)) if isinstance(axis, (list, tuple)) else int(axis))
        return Tensor(fn(_raw(input_tensor), axis=ax, keepdims=keepdims))
    return op


reduce_max, reduce_min, reduce_sum, reduce_mean = _reduce(np.max), _reduce(np.min), _reduce(np.sum), _reduce(np.mean)


def _binary(fn):
    def op(x, y, name=None):
        return Tensor(fn(_raw(x), _raw(y)))
    return op


def _unary(fn):
    def op(x, name=None):
        return Tensor(fn(_raw(x)))
    return op


maximum, minimum = _binary(np.maximum), _binary(np.minimum)
multiply, subtract, add, divide = _binary(np.multiply), _binary(np.subtract), _binary(np.add), _binary(np.true_divide)
floormod, floordiv = _binary(np.mod), _binary(np.floor_divide)
less, less_equal, greater, greater_equal, equal = (_binary(f) for f in (np.less, np.less_equal, np.greater, np.greater_equal, np.equal))
logical_and = _binary(np.logical_and)
square, sqrt, tanh, exp = _unary(np.square), _unary(np.sqrt), _unary(np.tanh), _unary(np.exp)


def relu(features, name=None):
    return Tensor(np.maximum(_raw(features), 0))


def elu(features, name=None):
    v = _raw(features)
    return Tensor(np.where(v > 0, v, np.expm1(np.minimum(v, 0))))


def sigmoid(x, name=None):
    return Tensor(1.0 / (1.0 + np.exp(-_raw(x))))


def softmax(logits, axis=None, name=None):
    v = _raw(logits)
    axis = -1 if axis is None else int(axis)
    e = np.exp(v - v.max(axis=axis, keepdims=True))
    return Tensor(e / e.sum(axis=axis, keepdims=True))


def matmul(a, b, name=None):
    a, b = _raw(a), _raw(b)
    if a.ndim != 2 or b.ndim != 2:
        raise NotImplementedError("matmul: rank 2 only")
    return Tensor(a @ b)


def tensordot(a, b, axes, name=None):
    return Tensor(np.tensordot(_raw(a), _raw(b), axes=axes))


def bias_add(value, bias, data_format=None, name=None):
    v, b = _raw(value), _raw(bias)
    if data_format not in (None, "NHWC") or b.ndim != 1 or b.shape[0] != v.shape[-1]:
        raise ValueError("bias_add: bias must be [last dimension of value]")
    return Tensor(v + b)


def _same(size, k, s):
    """TensorFlow SAME: output ceil(size / s); total padding max((out - 1) s + k - size, 0), the smaller half in front"""
    out = -(-size // s)
    total = max((out - 1) * s + k - size, 0)
    return out, total // 2, total - total // 2


def _nhwc_strides(strides, what):
    st = _ints(strides)
    if len(st) != 4 or st[0] != 1 or st[3] != 1:
        raise NotImplementedError(f"{what}: strides {st}")
    return st[1], st[2]


def conv2d(input, filter=None, strides=None, padding=None, use_cudnn_on_gpu=True, data_format="NHWC", dilations=[1, 1, 1, 1], name=None,
           filters=None):
    if filters is not None:
        if filter is not None:
            raise ValueError("conv2d: filter and filters")
        filter = filters
    if padding != "SAME" or data_format != "NHWC" or list(dilations) != [1, 1, 1, 1]:
        raise NotImplementedError(f"conv2d: padding {padding!r}, data_format {data_format!r}, dilations {dilations!r}")
    x, w = _raw(input), _raw(filter)
    sy, sx = _nhwc_strides(strides, "conv2d")
    B, H, W, C = x.shape
    kh, kw, ci, co = w.shape
    if ci != C:
        raise ValueError(f"conv2d: input has {C} channels, the filter reads {ci}")
    Ho, top, bottom = _same(H, kh, sy)
    Wo, left, right = _same(W, kw, sx)
    xp = np.zeros((B, H + top + bottom, W + left + right, C), np.float64)
    xp[:, top:top + H, left:left + W] = x
    out = np.zeros((B, Ho, Wo, co), np.float64)
    for ky in range(kh):
        for kx in range(kw):
            patch = xp[:, ky:ky + (Ho - 1) * sy + 1:sy, kx:kx + (Wo - 1) * sx + 1:sx]
            out += np.tensordot(patch, w[ky, kx], axes=([3], [0]))
    return Tensor(out)


def conv2d_transpose(value=None, filter=None, output_shape=None, strides=None, padding="SAME", data_format="NHWC", name=None, input=None,
                     filters=None, dilations=None):
    """the transpose (gradient with respect to its input) of conv2d(SAME): that convolution reads, for its output position o and
    filter tap k, its input at o * stride + k - pad_before; so here every input element x[o] is SCATTERED to o * stride + k - pad_before
    with the filter tap k, contracted over the filter's LAST axis.  filter [kh, kw, out channels, in channels]."""
    if padding != "SAME" or data_format != "NHWC" or dilations is not None:
        raise NotImplementedError(f"conv2d_transpose: padding {padding!r}, data_format {data_format!r}, dilations {dilations!r}")
    x = _raw(value if value is not None else input)
    w = _raw(filter if filter is not None else filters)
    sy, sx = _nhwc_strides(strides, "conv2d_transpose")
    B, h, wd, ci = x.shape
    kh, kw, co, ci2 = w.shape
    oB, Ho, Wo, oC = _ints(output_shape)
    if ci2 != ci:
        raise ValueError(f"conv2d_transpose: input has {ci} channels, the filter's last axis {ci2}")
    if oC != co:
        raise ValueError(f"conv2d_transpose: output_shape asks for {oC} channels, the filter writes {co}")
    if oB != B:
        raise ValueError("conv2d_transpose: batch size")
    fh, top, _ = _same(Ho, kh, sy)                          # the forward convolution over the OUTPUT's shape
    fw, left, _ = _same(Wo, kw, sx)
    if (fh, fw) != (h, wd):
        raise ValueError(f"conv2d_transpose: output_shape {Ho}x{Wo} does not convolve (stride {sy}x{sx}) to the input's {h}x{wd}")
    buf = np.zeros((B, max((h - 1) * sy + kh, top + Ho), max((wd - 1) * sx + kw, left + Wo), co), np.float64)
    for ky in range(kh):
        for kx in range(kw):
            buf[:, ky:ky + (h - 1) * sy + 1:sy, kx:kx + (wd - 1) * sx + 1:sx] += np.tensordot(x, w[ky, kx], axes=([3], [1]))
    return Tensor(buf[:, top:top + Ho, left:left + Wo])


def _pool(value, ksize, strides, padding, data_format, how):
    if padding != "SAME" or data_format != "NHWC":
        raise NotImplementedError(f"{how}_pool2d: padding {padding!r}, data_format {data_format!r}")
    x = _raw(value)
    ky, kx = _nhwc_strides(ksize, "pool ksize")
    sy, sx = _nhwc_strides(strides, "pool")
    B, H, W, C = x.shape
    Ho, top, bottom = _same(H, ky, sy)
    Wo, left, right = _same(W, kx, sx)
    fill = -np.inf if how == "max" else 0.0
    xp = np.full((B, H + top + bottom, W + left + right, C), fill, np.float64)
    xp[:, top:top + H, left:left + W] = x
    valid = np.zeros((1, H + top + bottom, W + left + right, 1), np.float64)
    valid[:, top:top + H, left:left + W] = 1
    out = np.full((B, Ho, Wo, C), fill, np.float64)
    cnt = np.zeros((1, Ho, Wo, 1), np.float64)
    for dy in range(ky):
        for dx in range(kx):
            sl = (slice(None), slice(dy, dy + (Ho - 1) * sy + 1, sy), slice(dx, dx + (Wo - 1) * sx + 1, sx))
            out = np.maximum(out, xp[sl]) if how == "max" else out + xp[sl]
            cnt += valid[sl]
    return Tensor(out if how == "max" else out / cnt)        # average: over the elements inside the image only


def max_pool2d(input, ksize, strides, padding, data_format="NHWC", name=None):
    return _pool(input, ksize, strides, padding, data_format, "max")


def avg_pool2d(input, ksize, strides, padding, data_format="NHWC", name=None):
    return _pool(input, ksize, strides, padding, data_format, "avg")


# ---------------------------------------------------------------------------------------------------------------------------
# control flow
# ---------------------------------------------------------------------------------------------------------------------------
def map_fn(fn, elems, dtype=None, parallel_iterations=None, back_prop=True, swap_memory=False, infer_shape=True, name=None):
    single = not isinstance(elems, (tuple, list))
    seqs = [_raw(elems)] if single else [_raw(e) for e in elems]
    n = seqs[0].shape[0]
    if n == 0 or any(s.shape[0] != n for s in seqs):
        raise NotImplementedError("map_fn: an empty or ragged first axis")
    outs = []
    for i in range(n):
        arg = Tensor(seqs[0][i]) if single else tuple(Tensor(s[i]) for s in seqs)
        outs.append(fn(arg))
    if isinstance(outs[0], (tuple, list)):
        if dtype is None or len(dtype) != len(outs[0]):
            raise ValueError("map_fn: fn returns a tuple, dtype must list its members")
        return tuple(stack([o[k] for o in outs]) for k in range(len(outs[0])))
    return stack(outs)


def while_loop(cond, body, loop_vars, shape_invariants=None, parallel_iterations=10, back_prop=True, swap_memory=False, name=None,
               maximum_iterations=None):
    state = list(loop_vars)
    for _ in range(1000000):
        if not bool(Tensor(cond(*state))):
            return state
        state = list(body(*state))
        if len(state) != len(loop_vars):
            raise ValueError("while_loop: the body returns another number of loop variables")
    raise RuntimeError("while_loop does not end")


# ---------------------------------------------------------------------------------------------------------------------------
# the modules
# ---------------------------------------------------------------------------------------------------------------------------
class _Strict(types.ModuleType):
    def __getattr__(self, item):
        if item.startswith("__") and item.endswith("__"):
            raise AttributeError(item)
        raise NotImplementedError(f"tf_eager_standin: {self.__name__}.{item} is not implemented")


class _Unimplemented:
    """a name the reference imports at module level but never uses on the paths that run here"""
    def __init__(self, name):
        self.__dict__["_name"] = name

    def __call__(self, *a, **k):
        raise NotImplementedError(f"tf_eager_standin: {self._name} is not implemented")

    def __getattr__(self, item):
        if item.startswith("__") and item.endswith("__"):
            raise AttributeError(item)
        raise NotImplementedError(f"tf_eager_standin: {self._name}.{item} is not implemented")


class _Refuse(importlib.abc.MetaPathFinder):
    """a tensorflow submodule this file does not provide: an ImportError, never somebody else's placeholder"""
    def find_spec(self, fullname, path, target=None):
        if fullname == "tensorflow" or fullname.startswith("tensorflow."):
            raise ImportError(f"tf_eager_standin provides no module {fullname}")
        return None


def _module(name, **members):
    m = _Strict(name)
    m.__path__ = []
    for k, v in members.items():
        setattr(m, k, v)
    return m


def _tf_export(*names, **kw):
    return lambda fn: fn


def build_modules():
    v1 = _module("tensorflow.compat.v1", variable_scope=variable_scope, get_variable=get_variable, get_variable_scope=get_variable_scope,
                 AUTO_REUSE=AUTO_REUSE)
    compat = _module("tensorflow.compat", v1=v1)
    nn = _module("tensorflow.nn", relu=relu, elu=elu, sigmoid=sigmoid, tanh=tanh, softmax=softmax, bias_add=bias_add, conv2d=conv2d,
                 conv2d_transpose=conv2d_transpose, max_pool2d=max_pool2d, avg_pool2d=avg_pool2d)
    math = _module("tensorflow.math", maximum=maximum, minimum=minimum, reduce_mean=reduce_mean, reduce_max=reduce_max, reduce_sum=reduce_sum,
                   square=square, sqrt=sqrt, subtract=subtract, divide=divide, multiply=multiply, floormod=floormod, floordiv=floordiv,
                   tanh=tanh)
    sparse = _module("tensorflow.sparse", reorder=_sparse_reorder, transpose=_sparse_transpose, softmax=_sparse_softmax,
                     reduce_sum=lambda sp_input, axis=None, keepdims=None: _sparse_reduce(sp_input, axis, "sum"),
                     reduce_max=lambda sp_input, axis=None, keepdims=None: _sparse_reduce(sp_input, axis, "max"))
    sets = _module("tensorflow.sets", difference=_sets_difference)
    random = _module("tensorflow.random", truncated_normal_initializer=_Initializer)
    cudnn = _module("tensorflow.contrib.cudnn_rnn", **{n: _Unimplemented(n) for n in
                                                         ("CudnnCompatibleLSTMCell", "CudnnCompatibleGRUCell", "CudnnLSTM", "CudnnGRU")})
    clayers = _module("tensorflow.contrib.layers", batch_norm=_Unimplemented("contrib.layers.batch_norm"))
    contrib = _module("tensorflow.contrib", cudnn_rnn=cudnn, layers=clayers)
    export = _module("tensorflow.python.util.tf_export", tf_export=_tf_export)
    util = _module("tensorflow.python.util", tf_export=export)
    framework = _module("tensorflow.python.framework", ops=_Unimplemented("python.framework.ops"))
    pops = _module("tensorflow.python.ops", control_flow_ops=_Unimplemented("python.ops.control_flow_ops"),
                   math_ops=_Unimplemented("python.ops.math_ops"))
    python = _module("tensorflow.python", util=util, framework=framework, ops=pops)
    tf = _module(
        "tensorflow", compat=compat, nn=nn, math=math, sparse=sparse, sets=sets, random=random, contrib=contrib, python=python,
        float32=float32, float64=float64, int32=int32, int64=int64, bool=bool_, AUTO_REUSE=AUTO_REUSE,
        Tensor=Tensor, SparseTensor=SparseTensor, TensorShape=TensorShape,
        shape=shape, constant=constant, convert_to_tensor=convert_to_tensor, identity=identity, Print=Print, cast=cast, zeros=zeros, ones=ones,
        range=range_, stack=stack, unstack=unstack, concat=concat, split=split, add_n=add_n, reshape=reshape, transpose=transpose,
        expand_dims=expand_dims, squeeze=squeeze, tile=tile, reverse=reverse, slice=slice_, gather=gather, gather_nd=gather_nd, where=where,
        sequence_mask=sequence_mask, unique=unique, reduce_max=reduce_max, reduce_min=reduce_min, reduce_sum=reduce_sum,
        reduce_mean=reduce_mean, maximum=maximum, minimum=minimum, multiply=multiply, subtract=subtract, add=add, divide=divide,
        less=less, less_equal=less_equal, greater=greater, greater_equal=greater_equal, equal=equal, logical_and=logical_and,
        square=square, sqrt=sqrt, tanh=tanh, exp=exp, matmul=matmul, tensordot=tensordot, map_fn=map_fn, while_loop=while_loop,
        name_scope=name_scope, random_normal_initializer=_Initializer, constant_initializer=_Initializer)
    return [tf, compat, v1, nn, math, sparse, sets, random, contrib, cudnn, clayers, python, util, export, framework, pops]


def install():
    if isinstance(sys.modules.get("tensorflow"), _Strict):
        return sys.modules["tensorflow"]
    for name in [n for n in sys.modules if n == "tensorflow" or n.startswith("tensorflow.")]:
        del sys.modules[name]
    mods = build_modules()
    for m in mods:
        sys.modules[m.__name__] = m
    sys.meta_path.insert(0, _Refuse())
    return mods[0]


# ---------------------------------------------------------------------------------------------------------------------------
# self-checks (torch-CPU as the second opinion on the restated op semantics)
# ---------------------------------------------------------------------------------------------------------------------------
def self_check():
    import torch
    import torch.nn.functional as F
    rng = np.random.default_rng(0)

    def close(a, b, what):
        a, b = np.asarray(a), np.asarray(b)
        assert a.shape == b.shape, (what, a.shape, b.shape)
        assert np.max(np.abs(a - b)) <= 1e-12 * max(1.0, np.max(np.abs(b))), (what, float(np.max(np.abs(a - b))))

    def nchw(a):
        return torch.as_tensor(np.ascontiguousarray(np.transpose(a, (0, 3, 1, 2))))

    def nhwc(t):
        return np.transpose(t.numpy(), (0, 2, 3, 1))

    # conv2d, SAME, even and odd filters: torch on an explicitly padded input (before = (k - 1) // 2, the rest behind)
    for k in (3, 4, 1):
        x, w = rng.normal(size=(2, 7, 5, 3)), rng.normal(size=(k, k, 3, 4))
        b, a = (k - 1) // 2, (k - 1) - (k - 1) // 2
        want = F.conv2d(F.pad(nchw(x), (b, a, b, a)), torch.as_tensor(np.ascontiguousarray(np.transpose(w, (3, 2, 0, 1)))))
        close(conv2d(x, w, [1, 1, 1, 1], "SAME")._v, nhwc(want), f"conv2d k={k}")
    # conv2d_transpose: the adjoint of the forward convolution, <conv(u), x> == <u, conv_transpose(x)>, for odd and even output sizes
    for (Ho, Wo), k, s in (((13, 22), 3, 2), ((7, 11), 3, 2), ((4, 6), 3, 2), ((13, 22), 8, 8), ((16, 9), 4, 4), ((1, 2), 3, 2)):
        w = rng.normal(size=(k, k, 3, 5))
        u = rng.normal(size=(1, Ho, Wo, 3))
        fwd = conv2d(u, w, [1, s, s, 1], "SAME")._v
        x = rng.normal(size=fwd.shape)
        back = conv2d_transpose(x, w, [1, Ho, Wo, 3], [1, s, s, 1])._v
        close(np.sum(fwd * x), np.sum(u * back), f"conv2d_transpose adjoint {Ho}x{Wo} k={k} s={s}")
    # pools with ceil output: torch ceil_mode, the average over the valid elements only
    for hw in ((13, 22), (16, 9), (1, 3)):
        x = rng.normal(size=(1,) + hw + (3,))
        close(max_pool2d(x, [1, 2, 2, 1], [1, 2, 2, 1], "SAME")._v, nhwc(F.max_pool2d(nchw(x), 2, 2, ceil_mode=True)), f"max_pool {hw}")
        close(avg_pool2d(x, [1, 2, 2, 1], [1, 2, 2, 1], "SAME")._v,
              nhwc(F.avg_pool2d(nchw(x), 2, 2, ceil_mode=True, count_include_pad=False)), f"avg_pool {hw}")
    # sparse ops on a hand-made tensor:  [[., 1, 2], [3, ., .], [., -4, .]]
    sp = _sparse_reorder(SparseTensor([[2, 1], [0, 2], [1, 0], [0, 1]], [-4.0, 2.0, 3.0, 1.0], [3, 3]))
    close(sp.values._v, [1, 2, 3, -4], "sparse.reorder")
    tr = _sparse_transpose(sp, perm=[1, 0])
    close(tr.indices._v, [[0, 1], [1, 0], [1, 2], [2, 0]], "sparse.transpose indices")
    close(tr.values._v, [3, 1, -4, 2], "sparse.transpose values")
    e = np.exp([1.0, -4.0])
    close(_sparse_softmax(tr).values._v, [1, e[0] / e.sum(), e[1] / e.sum(), 1], "sparse.softmax")
    close(_sparse_reduce(sp, 0, "sum")._v, [3, -3, 2], "sparse.reduce_sum")
    close(_sparse_reduce(SparseTensor([[0, 1], [2, 1]], [-1.0, -4.0], [3, 3]), 0, "max")._v, [0, -1, 0], "sparse.reduce_max")
    # integer helpers
    y, idx = unique([7, 3, 7, 9, 3])
    close(y._v, [7, 3, 9], "unique values")
    close(idx._v, [0, 1, 0, 2, 1], "unique idx")
    close(_sets_difference([[5, 1, 9, 4]], [[4, 0]]).values._v, [1, 5, 9], "sets.difference")
    close(gather_nd(np.arange(24).reshape(2, 3, 4), [[1, 2], [0, 0]])._v, [[20, 21, 22, 23], [0, 1, 2, 3]], "gather_nd")
    close(sequence_mask([2, 0, 3])._v, [[1, 1, 0], [0, 0, 0], [1, 1, 1]], "sequence_mask")
    # the variable store: sharing needs reuse, as in TF 1.x
    VARIABLES.reset(lambda name, shp: np.zeros(shp))
    with variable_scope("a") as sc:
        get_variable("w", [2, 3.0], initializer=_Initializer())
        try:
            get_variable("w", [2, 3], initializer=_Initializer())
        except ValueError:
            pass
        else:
            raise AssertionError("a second get_variable without reuse must raise")
        sc.reuse_variables()
        with variable_scope("b"):
            try:
                get_variable("new", [1], initializer=_Initializer())
            except ValueError:
                pass
            else:
                raise AssertionError("a new variable under reuse=True must raise")
        get_variable("w", [2, 3], initializer=_Initializer())
    with variable_scope("a", reuse=AUTO_REUSE):
        with variable_scope("c"):
            get_variable("v", 4, initializer=_Initializer())
            get_variable("v", 4, initializer=_Initializer())
    assert list(VARIABLES.created) == ["a/w", "a/c/v"], list(VARIABLES.created)
    VARIABLES.reset(None)
    return True
