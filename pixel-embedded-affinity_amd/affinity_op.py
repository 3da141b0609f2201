"""Host side of the hot path: descriptor construction, argument checking, autograd glue.

PyTorch is plumbing here (device memory, streams, autograd bookkeeping); all arithmetic happens in
libpea_hip.so through the C ABI of include/pea.h.  Nothing in this file has a CPU implementation:
tensors that are not on a ROCm device raise, and a missing library raises PeaLibraryError.

Reference behaviour mirrored (file:line in the reference tree):
  * embedding_loss / ema_embedding_loss / embedding2affs      scripts_cvppp/loss/loss_embedding_mse.py:18-95
  * embedding_loss_norm1/5, ema_*, inf_*                        scripts_ac3ac4/loss/loss_embedding_mse.py:7-289
  * WeightedMSE normaliser                                      scripts_cvppp/loss/loss.py:112-119
"""
import collections
import collections.abc
import ctypes
import operator
import os
import threading

import torch

from . import _lib
from ._lib import PeaDesc

SPECIALISED_TRAIN_D = (4, 8, 16, 32, 64)  # every other width trains through the runtime-D backward (REPLICATE border excepted)


class AffinitySpec(object):
    """Everything about one call that is not a tensor."""

    def __init__(self, ndim, offsets, lam, border, norm, eps=1e-12, relu=False, act=0):
        self.ndim = int(ndim)
        self.offsets = [tuple([0] * (3 - len(o)) + [int(v) for v in o]) for o in offsets]
        self.K = len(self.offsets)
        if not 1 <= self.K <= _lib.PEA_MAX_K:
            raise ValueError("number of offsets must be in 1..%d, got %d" % (_lib.PEA_MAX_K, self.K))
        self.lam = [1.0] * self.K if lam is None else [float(v) for v in lam]
        if len(self.lam) != self.K:
            raise ValueError("lambda list must have one entry per offset")
        self.border, self.norm, self.eps = border, norm, float(eps)
        # _lib.FLAG_* activation bits of the affs output; the loss uses the raw cosine unless FLAG_LOSS_ACT comes with them
        self.act = int(act)
        self.relu = bool(relu) or bool(self.act & _lib.FLAG_RELU_AFFS)

    @property
    def relu(self):
        return bool(self.act & _lib.FLAG_RELU_AFFS)

    @relu.setter
    def relu(self, on):
        self.act = (self.act | _lib.FLAG_RELU_AFFS) if on else (self.act & ~_lib.FLAG_RELU_AFFS)


def _spatial(e, ndim):
    if e.dim() != ndim + 2:
        raise ValueError("embedding must be %s, got shape %s" % ("[B,D,H,W]" if ndim == 2 else "[B,D,Z,Y,X]", tuple(e.shape)))
    sp = list(e.shape[2:])
    return [1] * (3 - len(sp)) + sp


def _require_gpu(t, name):
    if not isinstance(t, torch.Tensor):
        raise TypeError("%s must be a torch.Tensor" % name)
    if not t.is_cuda:
        raise RuntimeError("%s is on %s: the affinity path runs on an MI355X only (no CPU fallback)" % (name, t.device))


# storage dtype of the embedding -> PeaDesc.dtype (include/pea.h PEA_F32 / PEA_F16 / PEA_BF16)
_DTYPE_CODE = {torch.float32: _lib.F32, torch.float16: _lib.F16, torch.bfloat16: _lib.BF16}


def _embedding_arg(t, name):
    _require_gpu(t, name)
    if t.dtype not in _DTYPE_CODE:
        raise TypeError("%s must be float32, float16 or bfloat16, got %s" % (name, t.dtype))
    return t if t.is_contiguous() else t.contiguous()


def _batch_layout(t, name, dtype, shape):
    """-> (tensor, batch stride in elements): the layout decision of _batch_strided, which needs no device (CPU tensors pass).
    The library reads item b of a [B, K, spatial...] operand at data_ptr + b * (stride or K * S) elements as one dense [K, S] block
    (include/pea.h: a *_bstride of 0 means "dense"), so what comes back is
      * the tensor itself, with its own batch stride, where every item is such a block and the batch stride is positive: a channel
        slice of a packed tensor, t[::2], overlapping read-only windows from as_strided (0 < stride < K * S) -- no copy;
      * a dense copy with stride K * S for every other layout: a broadcast batch (stride(0) == 0 with B > 1 -- the descriptor has no
        encoding for it, 0 is taken: it means dense), an expanded channel, a spatial crop, channels_last, a permuted view;
      * stride 0 and a dense tensor for B == 1 (the stride is never used)."""
    if not isinstance(t, torch.Tensor):
        raise TypeError("%s must be a torch.Tensor" % name)
    if tuple(t.shape) != tuple(shape):
        raise ValueError("%s has shape %s, expected %s" % (name, tuple(t.shape), tuple(shape)))
    if t.dtype != dtype:
        t = t.to(dtype)
    if t.shape[0] <= 1:
        return (t if t.is_contiguous() else t.contiguous()), 0
    if t.stride(0) <= 0 or not t[0].is_contiguous():
        t = t.contiguous()
    return t, t.stride(0)


def _batch_strided(t, name, dtype, shape):
    """-> (tensor, batch stride in elements) of a device tensor: _batch_layout behind the device check.  The [K, spatial...] block of
    every batch item must be dense (it is copied otherwise); a positive batch stride is taken as it is (channel slices of a packed
    tensor); a batch stride of 0 (a tensor expanded over the batch) is materialised."""
    _require_gpu(t, name)
    return _batch_layout(t, name, dtype, shape)


def mask_arg(m, shape, gpu=True):
    """-> (mask, batch stride in elements, descriptor flag of its type).  A float32 mask goes to the kernels as it is
    (PEA_FLAG_MASK_F32: fractional values are honoured, as the reference's `affs * mask` after `mask.float()` does); other floating
    dtypes are converted once with .float(); bool / uint8 masks take the u8 path (other integer dtypes are converted to uint8).
    The layout is _batch_layout's; gpu=False leaves the device check out (the layout decision alone, on any tensor)."""
    if m is None:
        return None, 0, 0
    layout = _batch_strided if gpu else _batch_layout
    if m.dtype == torch.bool:
        m = m.view(torch.uint8)
    if m.is_floating_point():
        m, ms = layout(m, "mask", torch.float32, shape)
        return m, ms, _lib.FLAG_MASK_F32
    m, ms = layout(m, "mask", torch.uint8, shape)
    return m, ms, 0


_DESC_CACHE = {}


def make_desc(spec, e, tstride=0, wstride=0, mstride=0, mflag=0):
    """PeaDesc for `spec` on a tensor shaped like e (mflag: _lib.FLAG_MASK_F32 for an f32 mask, see mask_arg).  Descriptors are
    immutable once built (the library takes them as const), so they are memoised: filling and validating one costs more host time
    than the launch it describes."""
    key = (spec.ndim, tuple(spec.offsets), tuple(spec.lam), spec.border, spec.norm, spec.eps, spec.act, tuple(e.shape),
           e.dtype, int(tstride), int(wstride), int(mstride), int(mflag))
    d = _DESC_CACHE.get(key)
    if d is not None:
        return d
    if len(_DESC_CACHE) > 512:
        _DESC_CACHE.clear()
        _CROSS_OK.clear()  # (keyed by the identity of descriptors that are about to go away)
    d = _DESC_CACHE[key] = _build_desc(spec, e, tstride, wstride, mstride, mflag)
    return d


_CROSS_LOCK = threading.Lock()


class _IdMemo(object):
    """answers remembered by the IDENTITY of the objects they are about (memoised descriptors: comparing their bytes would cost what
    the memo saves).  The key is the objects' ids plus `extra`; an id can be reused once its object is gone, so the entry pins the
    objects, and a hit counts only if every pinned object `is` the one asked about.  More than `cap` entries clear the memo;
    insertion and clearing happen under the one lock (nn.DataParallel replicas ask from one thread per device)."""

    def __init__(self, cap):
        self.cap, self._d = cap, {}

    def get(self, objs, extra, compute):
        """compute() for the tuple `objs` and the hashable `extra`, remembered"""
        key = (*map(id, objs), extra)
        hit = self._d.get(key)
        if hit is None or not all(map(operator.is_, hit[1], objs)):
            r = compute()
            with _CROSS_LOCK:
                if len(self._d) > self.cap:
                    self._d.clear()
                self._d[key] = hit = (r, objs)
        return hit[0]

    def clear(self):
        with _CROSS_LOCK:
            self._d.clear()

    def __len__(self):
        return len(self._d)


_CROSS_OK = _IdMemo(2048)
_lib._RELOAD_HOOKS.append(_CROSS_OK.clear)  # pea_cross_supported depends on the PEA_* switches


def cross_supported(d, mode):
    """pea_cross_supported(desc, mode), remembered per memoised descriptor AND current device (the host-side plan behind it costs a few
    microseconds; the march kernels' answer depends on the device's CU count, and nn.DataParallel replicas call this from one thread
    per device: round-4 advice)"""
    return _CROSS_OK.get((d,), (mode, torch.cuda.current_device()), lambda: bool(_lib.lib().pea_cross_supported(ctypes.byref(d), mode)))


def _build_desc(spec, e, tstride, wstride, mstride, mflag=0):
    dims = _spatial(e, spec.ndim)
    d = PeaDesc()
    d.abi, d.ndim, d.B, d.D = _lib.PEA_ABI_VERSION, spec.ndim, e.shape[0], e.shape[1]
    d.dims[:] = dims
    d.K = spec.K
    d.border, d.norm, d.eps = spec.border, spec.norm, spec.eps
    d.dtype = _DTYPE_CODE[e.dtype]
    d.flags = spec.act | int(mflag)
    for i, o in enumerate(spec.offsets):
        if spec.border == _lib.BORDER_CIRCULAR:  # torch.roll is modular: fold into (-dim, dim)
            o = tuple(int(v) - dims[a] * int(int(v) / dims[a]) if dims[a] else 0 for a, v in enumerate(o))
        d.offsets[i][:] = o
        d.lam[i] = spec.lam[i]
    d.target_bstride, d.weight_bstride, d.mask_bstride = int(tstride), int(wstride), int(mstride)
    rc = _lib.lib().pea_desc_validate(ctypes.byref(d))
    if rc:
        raise ValueError("invalid affinity descriptor: %s" % _lib.lib().pea_strerror(rc).decode())
    return d


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


_RAW_STREAM = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def _stream():
    """the current HIP stream of the current device as a void*.  torch.cuda.current_stream() builds a Stream object through
    ~35 us of Python (device-index parsing); the raw handle is one C call -- the Python path of a training step is ~160 us of
    host time against ~215 us of GPU time, so this matters for staying GPU-bound on a busy host"""
    if _RAW_STREAM is not None:
        return ctypes.c_void_p(_RAW_STREAM(torch.cuda.current_device()))
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


_WS = {}
_RETIRED = []
_STATE_BYTES = [0]


def stream_workspace(family, dev, nb, init, name):
    """the workspace block of `family` (any hashable: a name, or a name and a count) for the CURRENT stream of `dev`, at least nb
    bytes: one block per (family, device, stream), allocated and prepared once with init(ptr, bytes, stream) -- `name` is what an
    error calls it -- on that stream, then reused by every call: each call leaves its block ready for the next one, and calls on one
    stream cannot overlap.  A call that needs more gets a larger block; the smaller one is retired, not freed, because a captured
    graph may still replay on it."""
    idx = dev.index if dev.index is not None else torch.cuda.current_device()
    raw = _RAW_STREAM(idx) if _RAW_STREAM is not None else torch.cuda.current_stream(dev).cuda_stream
    key = (family, idx, raw)
    w = _WS.get(key)
    if w is None or w.numel() * 4 < nb:
        if w is not None:
            _RETIRED.append(w)
        w = torch.empty(nb // 4, dtype=torch.float32, device=dev)
        _lib.check(init(ctypes.c_void_p(w.data_ptr()), nb, ctypes.c_void_p(raw)), name)
        _WS[key] = w
    return w


def _no_init(_ptr_, _bytes, _stream_):
    """the `init` of a stream_workspace that is scratch (pea_cc_label, pea_ws_seeds, pea_ws_flood): it needs no preparation"""
    return 0


def workspace(dev, desc, nstates=1):
    """(tensor, bytes): the loss-state block(s) of the training forward for the CURRENT stream of `dev` (include/pea.h,
    pea_workspace_bytes), ~16 KB per state: the stream_workspace of ("loss", nstates)."""
    L = _lib.lib()
    if not _STATE_BYTES[0]:
        _STATE_BYTES[0] = int(L.pea_workspace_bytes(ctypes.byref(desc)))
    nb = _STATE_BYTES[0] * nstates
    return stream_workspace(("loss", nstates), dev, nb, L.pea_workspace_init, "pea_workspace_init"), nb


class _on_device(object):
    """`with torch.cuda.device(dev)` without its cost when dev is already the current device (the one-process-per-GPU case)"""
    __slots__ = ("_ctx",)

    def __init__(self, dev):
        self._ctx = None if dev.index is None or dev.index == torch.cuda.current_device() else torch.cuda.device(dev)

    def __enter__(self):
        if self._ctx is not None:
            self._ctx.__enter__()

    def __exit__(self, *a):
        if self._ctx is not None:
            return self._ctx.__exit__(*a)
        return False


def _affs_shape(e, K):
    return (e.shape[0], K) + tuple(e.shape[2:])


def _pair_args(e, e_other):
    """-> (e_c, o_c): the embedding and the second operand (the EMA embedding, or None) as the kernels take them: contiguous, the
    second in the first's dtype and shape"""
    e_c = _embedding_arg(e, "embedding")
    if e_other is None:
        return e_c, None
    o_c = _embedding_arg(e_other, "ema_embedding").to(e_c.dtype)
    if o_c.shape != e_c.shape:
        raise ValueError("ema_embedding shape %s != embedding shape %s" % (tuple(o_c.shape), tuple(e_c.shape)))
    return e_c, o_c


def _loss_operands(spec, e_c, target, weight, mask, dev=None):
    """-> (desc, target, weight, mask, kshape) of a tensor-form loss on e_c: the three [B, K, spatial...] operands in the layout the
    kernels read (_batch_strided, mask_arg) and the descriptor that carries their batch strides and the mask's type.
    dev: the device every operand must live on (the autograd nodes ask; the section nodes never did)"""
    kshape = _affs_shape(e_c, spec.K)
    t, ts = _batch_strided(target, "target", torch.float32, kshape)
    w, ws = _batch_strided(weight, "weightmap", torch.float32, kshape)
    m, ms, mflag = mask_arg(mask, kshape)
    if dev is not None:
        for x in (e_c, t, w, m):
            if x is not None and x.device != dev:
                raise RuntimeError("all operands must live on %s" % dev)
    return make_desc(spec, e_c, ts, ws, ms, mflag), t, w, m, kshape


def _backward_operands(spec, d, e_c, role):
    """-> (inv, raw_ok): what a training forward on descriptor d writes for its backward besides g.  role: 1 -- a self loss; 2 -- a
    cross loss whose second operand is detached; 0 -- anything else: nothing.
    inv: the 1 / norm plane of e, 4 bytes per pixel, which the cross backward (axis-aligned stencil) stages next to e -- for role 2
    two planes (e, e_other) --, allocated where those kernels cover the shape (pea_cross_supported modes 1 / 2), else None.
    raw_ok: the backward also reads the forward's RAW cosine map (modes 3 / 4: the projection-first kernels at D > 16, the z-march
    backward of 3D volumes; never on an activated map).  Only then is the map written for a loss whose map nobody asked for, and
    only then is it saved like an input -- autograd's version counter then catches an in-place edit of the returned map between
    forward and backward; saved everywhere it would turn a harmless affs.relu_() before backward() into a RuntimeError."""
    if not role or not cross_supported(d, role):
        return None, False
    shape = (e_c.shape[0],) + tuple(e_c.shape[2:])
    inv = torch.empty(shape if role == 1 else (2,) + shape, dtype=torch.float32, device=e_c.device)
    return inv, spec.act == 0 and cross_supported(d, 3 if role == 1 else 4)


def _check_trainable(spec, D):
    if D not in SPECIALISED_TRAIN_D and spec.border == _lib.BORDER_REPLICATE:
        raise NotImplementedError("the replicate-border backward needs D in %s (got %d)" % (SPECIALISED_TRAIN_D, D))


def _loss_rows(specs, dev):
    """[n, 1 + kmax] f32: row j takes loss j and its K_j per-offset parts"""
    return torch.empty((len(specs), 1 + max(sp.K for sp in specs)), dtype=torch.float32, device=dev)


def affinity_infer(e, e_other, spec):
    """affs [B,K,...] f32 = pea_affinity_infer (no autograd)."""
    e, e_other = _pair_args(e, e_other)
    with _on_device(e.device):
        d = make_desc(spec, e)
        affs = torch.empty(_affs_shape(e, spec.K), dtype=torch.float32, device=e.device)
        _lib.check(_lib.lib().pea_affinity_infer(ctypes.byref(d), _ptr(e.detach()), _ptr(None if e_other is None else e_other.detach()),
                                                 _ptr(affs), _stream()), "pea_affinity_infer")
    return affs


# element type of a rules table -> PEA_RULES_* (include/pea_flip.h); every other dtype is converted once on the device
UNFLIP_DTYPES = tuple(_DTYPE_CODE)  # what pea_consistency_unflip moves: the embedding's storage dtypes
_RULES_CODE = {torch.uint8: _lib.RULES_U8, torch.int32: _lib.RULES_I32, torch.int64: _lib.RULES_I64, torch.float32: _lib.RULES_F32}


def check_unflip_shapes(t_shape, rules_shape):
    """the shapes unflip() and harness.train_step.convert_consistency_flip accept: a [B, C, H, W] or [B, C, Z, H, W] tensor with
    [B, 3] rules (x-flip, y-flip, xy-transpose), or a [B, C, Z, H, W] tensor with [B, 4] rules (z-flip, x-flip, y-flip, xy-transpose)"""
    t_shape, rules_shape = tuple(t_shape), tuple(rules_shape)
    if len(t_shape) not in (4, 5):
        raise ValueError("the tensor must be [B,C,H,W] or [B,C,Z,H,W], got shape %s" % (t_shape,))
    if len(rules_shape) != 2 or rules_shape[1] not in (3, 4):
        raise ValueError("rules must be [B,3] or [B,4], got shape %s" % (rules_shape,))
    if rules_shape[1] == 4 and len(t_shape) != 5:
        raise ValueError("[B,4] rules (z-flip, x-flip, y-flip, xy-transpose) need a [B,C,Z,H,W] tensor, got shape %s" % (t_shape,))
    if rules_shape[0] != t_shape[0]:
        raise ValueError("rules has %d rows for a batch of %d" % (rules_shape[0], t_shape[0]))


def unflip(t, rules):
    """pea_consistency_unflip (include/pea_flip.h): the per-sample inverse of the EMA branch's flips / transpose in ONE launch, the
    rules read on the device (no host synchronisation: the call can be captured into a HIP graph and replayed on new rules).
    t [B,C,H,W] or [B,C,Z,H,W] f32 / f16 / bf16 on a ROCm device; rules a tensor on the same device, [B,3] = (x-flip, y-flip,
    xy-transpose) or, for a volume, [B,4] = (z-flip, x-flip, y-flip, xy-transpose); a rule is set when it is nonzero.
    Returns a NEW, detached, contiguous tensor: a bit-exact copy.  A sample whose transpose rule is set on a non-square plane comes
    back all NaN (the host cannot see the rules)."""
    _require_gpu(t, "tensor")
    if t.dtype not in _DTYPE_CODE:
        raise TypeError("the tensor must be float32, float16 or bfloat16, got %s" % t.dtype)
    _require_gpu(rules, "rules")
    check_unflip_shapes(t.shape, rules.shape)
    if rules.device != t.device:
        raise RuntimeError("rules is on %s, the tensor on %s" % (rules.device, t.device))
    t = t.detach()
    if not t.is_contiguous():
        t = t.contiguous()
    if rules.dtype == torch.bool:
        rules = rules.view(torch.uint8)
    elif rules.dtype not in _RULES_CODE:
        rules = rules.to(torch.float32 if rules.is_floating_point() else torch.int64)
    rules = rules.detach()
    if not rules.is_contiguous():
        rules = rules.contiguous()
    Z = t.shape[2] if t.dim() == 5 else 1
    with _on_device(t.device):
        out = torch.empty(t.shape, dtype=t.dtype, device=t.device)
        _lib.check(_lib.lib().pea_consistency_unflip(t.shape[0], t.shape[1], Z, t.shape[-2], t.shape[-1], _DTYPE_CODE[t.dtype], _ptr(t),
                                                     _ptr(out), _ptr(rules), _RULES_CODE[rules.dtype], rules.shape[1], _stream()),
                   "pea_consistency_unflip")
    return out


class FusedAffinityMSE(torch.autograd.Function):
    """loss, affs, per_offset_losses = f(e, e_other, target, weight, mask): the WeightedMSE criterion fused into the affinity
    forward.  One forward launch (saving g = d loss / d affs and, for the self loss, the 1 / norm plane of e) and one backward
    launch.  Despite its name it carries either criterion of the loss on the activated map: with FLAG_LOSS_ACT | FLAG_LOSS_BCE in
    spec.act the forward's epilogue takes the weighted binary cross-entropy instead of the squared residual (include/pea.h); the
    backward only ever sees g.  (Round 1 also had an opt-in one-launch step on this tensor path, PEA_FUSED=1; it sampled target / weight / mask at
    p and at p - o with one-dword loads, only ever tied the two launches and is gone -- the one-launch step that pays is the
    labels-in one, LabelsAffinityMSE below.)"""

    @staticmethod
    def forward(ctx, e, e_other, target, weight, mask, spec):
        ctx.set_materialize_grads(False)  # no 95 MB zero tensors for the gradients of the non-differentiable outputs
        e_c, o_c = _pair_args(e, e_other)
        if o_c is not None and o_c.device != e_c.device:
            raise RuntimeError("all operands must live on %s" % e_c.device)
        want_e = e.requires_grad
        want_o = e_other is not None and e_other.requires_grad
        with _on_device(e_c.device):
            d, target, weight, mask, kshape = _loss_operands(spec, e_c, target, weight, mask, e_c.device)
            L = _lib.lib()
            affs = torch.empty(kshape, dtype=torch.float32, device=e_c.device)
            loss_vec = torch.empty(1 + spec.K, dtype=torch.float32, device=e_c.device)
            work, wsb = workspace(e_c.device, d)
            # g = d loss / d affs is all the backward needs besides the embeddings; skip it when nothing trains
            g = torch.empty(kshape, dtype=torch.float32, device=e_c.device) if (want_e or want_o) else None
            inv, raw_ok = _backward_operands(spec, d, e_c, 0 if not want_e or want_o else 1 if o_c is None else 2)
            _lib.check(L.pea_affinity_fwd_ex(ctypes.byref(d), _ptr(e_c), _ptr(o_c), _ptr(target), _ptr(weight), _ptr(mask),
                                             _ptr(affs), _ptr(g), _ptr(inv), _ptr(loss_vec), _ptr(work), wsb, _stream()),
                       "pea_affinity_fwd_ex")
        ctx.spec, ctx.desc = spec, d
        ctx.has_other = o_c is not None
        ctx.save_for_backward(e_c, o_c, g, inv, affs if raw_ok else None)
        loss, per_offset = loss_vec[0], loss_vec[1:]  # views of a buffer that is not itself returned
        ctx.mark_non_differentiable(affs, per_offset)
        return loss, affs, per_offset

    @staticmethod
    def backward(ctx, dloss, _daffs, _dvec):
        e_c, o_c, g, inv, raw = ctx.saved_tensors
        want_e = ctx.needs_input_grad[0]
        want_o = ctx.has_other and ctx.needs_input_grad[1]
        if not (want_e or want_o) or dloss is None:
            return None, None, None, None, None, None
        _check_trainable(ctx.spec, e_c.shape[1])
        with _on_device(e_c.device):
            L = _lib.lib()
            dl = dloss.to(device=e_c.device, dtype=torch.float32).contiguous()
            de = torch.empty_like(e_c) if want_e else None
            de_o = torch.empty_like(o_c) if want_o else None
            _lib.check(L.pea_affinity_bwd_ex2(ctypes.byref(ctx.desc), _ptr(e_c), _ptr(o_c), _ptr(g), _ptr(inv), _ptr(raw), _ptr(dl),
                                              _ptr(de), _ptr(de_o), _stream()), "pea_affinity_bwd_ex2")
        return de, de_o, None, None, None, None


class MultiUnsupported(NotImplementedError):
    """the table of losses is outside the fused set of include/pea_multi.h (pea_multi_supported == 0: D other than 16 / 32, more than
    four losses or twelve offsets, a REPLICATE border, a loss on the activated map -- or embeddings of different dtypes: float32,
    float16 and bfloat16 tables are all fused, a table that mixes them is not), or it is a 16-bit table too large for the batched
    launch to pay (multi16_pays): nothing was launched, the *_multi wrappers and the sections make the single calls instead -- same
    results"""


_MULTI_OK = _IdMemo(256)


def multi_supported(descs):
    """pea_multi_supported for a list of memoised descriptors, remembered by their identities (host-only, but it validates each
    descriptor again: more host time than the launch it decides about)"""
    def ask():
        arr = (ctypes.POINTER(PeaDesc) * len(descs))(*[ctypes.pointer(d) for d in descs])
        return bool(_lib.lib().pea_multi_supported(arr, len(descs)))
    return _MULTI_OK.get(tuple(descs), (), ask)


# The tensor-form batched launches on 16-bit storage pay while the table is launch-sized.  Measured on an MI355X with bf16 embeddings
# (profiles/multi16_ab.json, cvppp_loss_section, gain of batched=True in us per step): at B = 2, 772 tiles of 256 pixels, it wins
# eager and ties graphed; at B = 8, 3088 tiles, it LOSES 40-60 us both ways -- there the call-by-call path runs the LDS-staged cross
# kernels (k_fwd_xdma_h / k_bwd_xdma_h) and the scales are no longer launch-sized, while the gather body pays one 2-byte load per
# lane and channel.  Nothing was measured in between, so the limit is the size up to which every workgroup of the launch is resident
# at once and the launch is latency-bound like the measured 772: 256 CUs x 4 workgroups (k_bwd_multi needs up to 116 VGPRs: four
# waves per SIMD, a workgroup puts one wave on each).  A 16-bit table above it is left to the single calls, so batched=True never
# costs more than it did before the 16-bit kernels existed.  f32 tables are taken as before at every size.  The labels-in form is
# not limited: at B = 8 it is as fast eager as the single calls on materialised label images which the same call ran before
# (395-396 us against 398-464) and 3-5 us slower graphed (393-395 against 390), inside the 7-8 us spread of that leg.
MULTI16_MAX_TILES = 1024


def multi16_pays(descs):
    """False for a table of 16-bit embeddings with more than MULTI16_MAX_TILES tiles (256 voxels of one batch item): op.MultiAffinityMSE
    then raises MultiUnsupported and the wrappers / sections make the single calls, which were measured to be faster there"""
    if descs[0].dtype == _lib.F32:
        return True
    tiles = sum(d.B * ((d.dims[0] * d.dims[1] * d.dims[2] + 255) // 256) for d in descs)
    return tiles <= MULTI16_MAX_TILES


def multi_backward(descs, e_cs, gs, dlosses):
    """de_j = dloss_j * d loss_j / d e_j of n self losses as ONE launch (pea_affinity_bwd_multi); dlosses: device scalars (or None = 1).
    de_j has the dtype of e_j (float32 / float16 / bfloat16, one for the whole table): a 16-bit de is the f32 result rounded once"""
    n = len(descs)
    des = [torch.empty_like(e_c) for e_c in e_cs]
    table = (_lib.PeaMultiBwd * n)()
    for j in range(n):
        a = table[j]
        a.desc, a.e, a.g, a.de = ctypes.pointer(descs[j]), e_cs[j].data_ptr(), gs[j].data_ptr(), des[j].data_ptr()
        a.dloss = None if dlosses[j] is None else dlosses[j].data_ptr()
    rc = _lib.lib().pea_affinity_bwd_multi(table, n, _stream())
    if rc == _lib.E_UNSUPPORTED:
        raise MultiUnsupported("pea_affinity_bwd_multi: the table is outside the fused set")
    _lib.check(rc, "pea_affinity_bwd_multi")
    return des


def multi_forward(specs, tensors, need_affs, rows, embs):
    """n self losses as ONE forward launch and one loss finish (pea_affinity_fwd_multi): loss j and its per-offset parts into
    rows[j] (rows=None: a block of its own) -> (descs, e_cs, gs, affs, rows), with g_j = d loss_j / d affs_j for multi_backward.
    specs: n AffinitySpecs; tensors: n (target, weight, mask) triples as FusedAffinityMSE takes them; need_affs=False: the maps are
    not written (empty tensors come back).  Embeddings: float32, float16 or bfloat16, all n of ONE dtype; maps, loss rows and g stay
    float32.  Raises MultiUnsupported, before anything is launched, where the table is outside the fused set."""
    n = len(embs)
    if not (len(specs) == len(tensors) == n):
        raise ValueError("one spec and one (target, weight, mask) triple per embedding")
    e_cs = [_embedding_arg(e, "embedding") for e in embs]
    dev = e_cs[0].device
    ops = [_loss_operands(spec, e_c, t, w, m, dev) for spec, e_c, (t, w, m) in zip(specs, e_cs, tensors)]
    descs = [a[0] for a in ops]
    if not 1 <= n <= _lib.PEA_MULTI_MAX_N or not multi_supported(descs):
        raise MultiUnsupported("the table is outside the fused set of include/pea_multi.h")
    if not multi16_pays(descs):
        raise MultiUnsupported("a 16-bit table of more than %d tiles: the single calls are faster (multi16_pays)" % MULTI16_MAX_TILES)
    with _on_device(dev):
        if rows is None:
            rows = _loss_rows(specs, dev).unbind(0)
        gs = [torch.empty(a[4], dtype=torch.float32, device=dev) for a in ops]  # (g_out is required by the C call)
        affs = [torch.empty(a[4] if need_affs else (0,), dtype=torch.float32, device=dev) for a in ops]
        work, wsb = workspace(dev, descs[0], n)
        table = (_lib.PeaMultiFwd * n)()
        for j in range(n):
            a, (d, t, w, m, _) = table[j], ops[j]
            a.desc, a.e, a.target, a.weight = ctypes.pointer(d), e_cs[j].data_ptr(), t.data_ptr(), w.data_ptr()
            a.mask = None if m is None else m.data_ptr()
            a.affs = affs[j].data_ptr() if need_affs else None
            a.g_out, a.loss_out = gs[j].data_ptr(), rows[j].data_ptr()
        rc = _lib.lib().pea_affinity_fwd_multi(table, n, _ptr(work), wsb, _stream())
    if rc == _lib.E_UNSUPPORTED:  # (nothing was launched)
        raise MultiUnsupported("pea_affinity_fwd_multi: the table is outside the fused set")
    _lib.check(rc, "pea_affinity_fwd_multi")
    return descs, e_cs, gs, affs, rows


class MultiAffinityMSE(torch.autograd.Function):
    """n self losses with the fused WeightedMSE as ONE node -- the four deep-supervision scales of a training step
    (scripts_cvppp/main.py:284-287, scripts_ac3ac4/main.py:227-230): one forward launch over every tile of every scale, one loss
    finish (multi_forward), one backward launch (multi_backward, with autograd's grad_outputs as the per-loss dloss) instead of
    three launches per scale (include/pea_multi.h).

        loss_0 .. loss_{n-1}, affs_0 .. affs_{n-1}, per_offset_0 .. per_offset_{n-1} = f(specs, tensors, need_affs, *embeddings)

    The arguments are multi_forward's; gradients take the embedding's dtype.  A caller that owns the weighting and the backward (the
    section nodes) calls multi_forward and multi_backward itself."""

    @staticmethod
    def forward(ctx, specs, tensors, need_affs, *embs):
        ctx.set_materialize_grads(False)
        n = len(embs)
        descs, e_cs, gs, affs, rows = multi_forward(specs, tensors, need_affs, None, embs)
        ctx.descs, ctx.n = descs, n
        if any(e.requires_grad for e in embs):
            ctx.save_for_backward(*(e_cs + gs))
        losses = [rows[j][0] for j in range(n)]
        parts = [rows[j][1:1 + specs[j].K] for j in range(n)]
        ctx.mark_non_differentiable(*(affs + parts))
        return tuple(losses) + tuple(affs) + tuple(parts)

    @staticmethod
    def backward(ctx, *grads):
        n = ctx.n
        # one launch over the losses that take part in this backward (a sub-table of a fused table is fused)
        live = [j for j in range(n) if grads[j] is not None and ctx.needs_input_grad[3 + j]]
        if not live:
            return (None, None, None) + (None,) * n
        saved = ctx.saved_tensors
        e_cs, gs = saved[:n], saved[n:]
        dev = e_cs[0].device
        with _on_device(dev):
            dls = [grads[j].to(device=dev, dtype=torch.float32).contiguous() for j in live]
            des = multi_backward([ctx.descs[j] for j in live], [e_cs[j] for j in live], [gs[j] for j in live], dls)
        out = [None] * n
        for j, de in zip(live, des):
            out[j] = de
        return (None, None, None) + tuple(out)


_ONES = {}


def backward(loss, **kw):
    """loss.backward() (scripts_cvppp/main.py:311) without its per-step fill kernel: autograd seeds the backward of a scalar with
    torch.ones_like(loss) -- a launch-bound 5 us kernel plus a kernel boundary between the loss forward and its backward, 3 % of a
    215 us step.  The seed is a constant: one cached ones-scalar per device is handed to backward() instead."""
    key = (loss.device, loss.dtype)
    one = _ONES.get(key)
    if one is None:
        one = _ONES[key] = torch.ones((), dtype=loss.dtype, device=loss.device)
    loss.backward(one, **kw)


class Graphed(object):
    """fn(*static_inputs) captured ONCE in a HIP graph; replay() runs it again on whatever the static input tensors hold now.

    Why: at small shapes the path is host-bound -- one 544 x 544 image through embedding_loss + backward is 0.12 ms of Python, ctypes and
    autograd bookkeeping around 0.05 ms of kernels (BASELINE configs[0]; the BBBC 256 x 256 training crops likewise).  Everything fn
    launches (the library's kernels through the C ABI, autograd's own kernels, allocations -- taken from the graph's private pool)
    becomes one graph launch of ~10 us of host time.  fn may contain the backward (pea.backward(loss)): gradients it leaves on leaf
    tensors are captured like any other output.

        E, T, W, M = ...                                   # static inputs: refill them with .copy_() between replays
        def step(E, T, W, M):
            E.grad = None
            loss, affs, _ = pea.embedding_loss(E, T, W, M, crit, offsets)
            pea.backward(loss)
            return loss, affs, E.grad
        g = pea.graphed(step, E, T, W, M)
        loss, affs, grad = g.replay()                      # the same tensors every time (overwritten by the next replay)

    The capture is bit-identical to the eager call (same kernels, same order; tests/test_gpu_parity.py::test_graphed_step_equals_eager).
    Constraints are those of torch.cuda.graph: static shapes and addresses, no host synchronisation inside fn (the path has none)."""

    def __init__(self, fn, *static_inputs, warmup=2):
        dev = next((t.device for t in static_inputs if isinstance(t, torch.Tensor) and t.is_cuda), None)
        if dev is None:
            raise RuntimeError("graphed() needs at least one static input on a ROCm device (no CPU fallback)")
        self.static_inputs = static_inputs
        with torch.cuda.device(dev):
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):  # warm-up on the capture stream: allocator, memoised descriptors, the stream's loss-state block
                for _ in range(max(1, warmup)):
                    fn(*static_inputs)
            torch.cuda.current_stream().wait_stream(side)
            torch.cuda.synchronize()
            self.graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self.graph, stream=side):
                self.outputs = fn(*static_inputs)

    def replay(self):
        self.graph.replay()
        return self.outputs

    __call__ = replay


def graphed(fn, *static_inputs, warmup=2):
    """Graphed(fn, *static_inputs): see there"""
    return Graphed(fn, *static_inputs, warmup=warmup)


class AffinityMap(torch.autograd.Function):
    """affs = f(e, e_other) with a true vjp, for criteria other than the fused WeightedMSE."""

    @staticmethod
    def forward(ctx, e, e_other, spec):
        e_c, o_c = _pair_args(e, e_other)
        affs = affinity_infer(e_c, o_c, spec)
        ctx.spec = spec
        ctx.has_other = o_c is not None
        ctx.save_for_backward(e_c, o_c)
        return affs

    @staticmethod
    def backward(ctx, d_affs):
        e_c, o_c = ctx.saved_tensors
        want_e = ctx.needs_input_grad[0]
        want_o = ctx.has_other and ctx.needs_input_grad[1]
        if not (want_e or want_o):
            return None, None, None
        if ctx.spec.act:
            raise NotImplementedError("an activation of the affs output is inference-only: apply it to the map yourself")
        _check_trainable(ctx.spec, e_c.shape[1])
        with _on_device(e_c.device):
            d = make_desc(ctx.spec, e_c)
            da = d_affs.to(torch.float32).contiguous()
            de = torch.empty_like(e_c) if want_e else None
            de_o = torch.empty_like(o_c) if want_o else None
            _lib.check(_lib.lib().pea_affinity_bwd(ctypes.byref(d), _ptr(e_c), _ptr(o_c), _ptr(da), None, _ptr(de), _ptr(de_o),
                                                   _stream()), "pea_affinity_bwd (vjp)")
        return de, de_o, None


class LossList(collections.abc.Sequence):
    """The reference's `all_loss` (a list of K Python floats filled by K `.item()` syncs,
    scripts_cvppp/loss/loss_embedding_mse.py:41) without the syncs: a read-only sequence whose floats are fetched from the
    device tensor on first access (one copy).  A Sequence, not a list subclass: C-level list operations would read the empty
    underlying storage of a lazily filled list (`all_loss + [x]`, `==`, copy, pickle); here every one of them goes through
    __getitem__ / __len__, and + / == against lists are defined to behave like the list the reference returns."""

    def __init__(self, dev_tensor):
        self.tensor = dev_tensor
        self._vals = None

    def _fill(self):
        if self._vals is None:
            self._vals = self.tensor.tolist()
        return self._vals

    def __len__(self):
        return self.tensor.numel()

    def __getitem__(self, i):
        return self._fill()[i]

    def __iter__(self):
        return iter(self._fill())

    def __repr__(self):
        return repr(self._fill())

    def __eq__(self, other):
        return list(self) == list(other) if isinstance(other, (list, tuple, LossList)) else NotImplemented

    def __add__(self, other):
        return list(self) + list(other)

    def __radd__(self, other):
        return list(other) + list(self)

    def __reduce__(self):
        return (list, (self._fill(),))  # copies / pickles as the plain list of floats


def labels_offsets_in_range(spec, e):
    """False when an offset reaches past the image (|o| >= dim): torch.roll folds such an offset modulo the dimension, which is
    what the tensor path's descriptor does, but the reference's gen_affs_ours (scripts_cvppp/utils/affinity_ours.py:17-39)
    shifts the LABEL image by the true offset -- every neighbour is then outside, mask 0, loss 0.  The labels-in kernels
    derive target / mask from the descriptor's (folded) offset, so they must not be used there: the *_from_labels wrappers
    fall back to gen_targets (true offsets) + the tensor path."""
    dims = _spatial(e, spec.ndim)
    return all(abs(o[a]) < dims[a] for o in spec.offsets for a in range(3))


ACTIVATIONS = {
    None: 0, "none": 0,
    "relu": _lib.FLAG_RELU_AFFS,                                   # F.relu(pred): scripts_cvppp/main.py:312, inference.py:193
    "mutex": _lib.FLAG_RELU_AFFS | _lib.FLAG_ONE_MINUS,            # 1 - relu(a): what seg_mutex hands to elf (utils/seg_mutex.py:4-5)
    "half": _lib.FLAG_HALF_SHIFT,                                  # (a + 1) / 2 = the L2 affinity 1 - |ehat_p - ehat_q|^2 / 4
    "half_clamp": _lib.FLAG_HALF_SHIFT | _lib.FLAG_CLAMP01,        # loss_embedding.py's embedding2affs: clamp((a + 1) / 2, 0, 1)
    "clamp": _lib.FLAG_CLAMP01,                                    # loss_embedding_exp.py's embedding2affs: clamp(a, 0, 1)
}


def activation_flags(activation):
    if isinstance(activation, int):
        return activation
    try:
        return ACTIVATIONS[activation]
    except KeyError:
        raise ValueError("activation must be one of %s (or FLAG_* bits), got %r" % (sorted(k for k in ACTIVATIONS if k), activation))


_RANGE_MSG = "label ids must fit int32 (and not be -2^31, the kernels' outside marker)%s: relabel the segmentation first"
_RANGE_CHECKS = collections.deque()  # (event, pinned flag) of range checks of GPU label tensors that have not been read back yet
_RANGE_LOCK = threading.Lock()       # the reference drives replicas from nn.DataParallel threads: the queue is shared


def check_label_ranges(block=True):
    """Read back the deferred range checks of _labels_int32 (GPU labels wider than int32): raises ValueError if an earlier label
    tensor held an id outside int32.  block=False only looks at checks whose copy has already arrived (no host sync); the
    labels-in entry points poll that way on every call, so a bad id surfaces one or two calls later at the latest."""
    while True:
        with _RANGE_LOCK:
            if not _RANGE_CHECKS:
                return
            ev, host = _RANGE_CHECKS[0]
            if not block and not ev.query():
                return
            _RANGE_CHECKS.popleft()
        ev.synchronize()
        if bool(host.item()):
            raise ValueError(_RANGE_MSG % " (found by the deferred range check of an earlier call)")


def _labels_int32(labels):
    """segmentation ids as the kernels take them (int32).  Wider ids are range-checked: a silent cast would turn an id >= 2^31
    negative (background for BOTH_FOREGROUND) and make ids that agree modulo 2^32 compare equal.  CPU tensors are checked at once;
    for GPU tensors the check runs on the device and its flag comes back through pinned memory without a host sync
    (check_label_ranges) -- ten blocking min / max round trips per training step was what the labels-in path was built to avoid.
    Under stream capture the check is skipped (a graph cannot raise): validate the ids where they are produced."""
    if labels.dtype in (torch.int64, torch.uint64) and labels.numel():
        l64 = labels.view(torch.int64) if labels.dtype == torch.uint64 else labels  # ids >= 2^63 come out negative: flagged too
        if not labels.is_cuda:
            lo, hi = int(l64.min()), int(l64.max())
            if lo <= -2 ** 31 or hi >= 2 ** 31:  # (-2^31 itself is the kernels' outside-the-image marker: include/pea.h)
                raise ValueError(_RANGE_MSG % (" (got %d .. %d)" % (lo, hi)))
        elif not torch.cuda.is_current_stream_capturing():
            check_label_ranges(block=False)
            top = l64 >> 31  # 0 or -1 for an id inside int32
            bad = (((top != 0) & (top != -1)) | (l64 == -2 ** 31)).any()  # (-2^31: the kernels' outside-the-image marker)
            # the flag starts out False (never garbage) and the event is recorded on the stream the copy was queued on: the current
            # stream of the LABELS' device, which need not be the current device
            host = torch.zeros((), dtype=torch.bool).pin_memory()
            with torch.cuda.device(labels.device):
                host.copy_(bad, non_blocking=True)
                ev = torch.cuda.Event()
                ev.record(torch.cuda.current_stream(labels.device))
            with _RANGE_LOCK:
                _RANGE_CHECKS.append((ev, host))
    return labels.to(torch.int32).contiguous()


LABELS_TWO_LAUNCH_MIN_PX = 1 << 18  # B * pixels from which the two-launch labels step (pea_affinity_fwd_bwd_labels_ex) pays


class LabelsStepUnsupported(NotImplementedError):
    """pea_affinity_fwd_bwd_labels has no kernel for the descriptor; the *_from_labels wrappers then generate the
    target / mask / weight tensors on the GPU (pea_gen_targets) and take the tensor path -- same results."""


class MultiLabelsUnsupported(NotImplementedError):
    """the table of labels-in losses is outside the fused set of include/pea_multi_labels.h (pea_multi_labels_supported == 0): nothing
    was launched, the *_from_labels_multi wrappers and the sections make the single calls on materialised label images instead"""


def label_sources(embs, ndim, labels, label_steps=None):
    """-> [(label tensor, (sz, sy, sx))] per embedding.  labels: a list with one label tensor per embedding, or ONE tensor all of
    them sample; label_steps: per embedding None, an int (the in-plane step: z keeps 1) or a tuple of ndim (or 3) steps.  A step of
    None is label size / embedding size, which must divide exactly on every axis (there OpenCV's nearest rule, src = floor(dst / f),
    is the plain stride); ValueError otherwise, and for a step that reads past the label image."""
    n = len(embs)
    shared = isinstance(labels, torch.Tensor)
    if not shared and len(labels) != n:
        raise ValueError("one label tensor per embedding (or one tensor for all)")
    if label_steps is not None and len(label_steps) != n:
        raise ValueError("one label step per embedding")
    out = []
    for j, e in enumerate(embs):
        lab = labels if shared else labels[j]
        if not isinstance(lab, torch.Tensor):
            raise TypeError("labels must be a torch.Tensor (or a list of them)")
        dims = _spatial(e, ndim)
        if lab.dtype.is_floating_point or lab.dim() != ndim + 1 or lab.shape[0] != e.shape[0]:
            raise ValueError("labels must be an integer tensor [B, %s] with the embedding's batch size, got %s for embedding %s"
                             % ("H, W" if ndim == 2 else "Z, Y, X", tuple(lab.shape), tuple(e.shape)))
        ldims = [1] * (3 - ndim) + list(lab.shape[1:])
        step = None if label_steps is None else label_steps[j]
        if step is None:
            if any(l % d for l, d in zip(ldims, dims)):
                raise ValueError("label image %s is no integer multiple of the embedding's %s: pass nearest-downsampled label images "
                                 "(label_downs / one label tensor per embedding) instead" % (tuple(ldims[3 - ndim:]), tuple(dims[3 - ndim:])))
            step = [l // d for l, d in zip(ldims, dims)]
        elif isinstance(step, int):
            step = [1, step, step]
        else:
            step = [1] * (3 - len(step)) + [int(v) for v in step]
        if any(v < 1 for v in step) or any((d - 1) * v + 1 > l for d, v, l in zip(dims, step, ldims)):
            raise ValueError("label step %s reads outside the label image %s for an embedding of %s" % (tuple(step), tuple(ldims), tuple(dims)))
        out.append((lab, tuple(step)))
    return out


def materialise_labels(lab, e, ndim, step):
    """the label image an embedding sees, as a tensor of its own: labels[b][z * sz][y * sy][x * sx]"""
    dims = _spatial(e, ndim)
    if all(v == 1 for v in step) and list(lab.shape[1:]) == dims[3 - ndim:]:
        return lab
    v = lab.unsqueeze(1) if ndim == 2 else lab
    v = v[:, ::step[0], ::step[1], ::step[2]][:, :dims[0], :dims[1], :dims[2]]
    return (v.squeeze(1) if ndim == 2 else v).contiguous()


def label_weight_table(d, lab, flags, B, K):
    """-> (wtab, counts, cb): the class-balance table [B, K, 2] of the int32 label image `lab` under descriptor d and the target
    flags (pea_label_weights: weight_binary_ratio per image and channel, one count launch), with the counts buffer it used"""
    counts, cb = label_counts(d, lab.device)
    wtab = torch.empty(B * K * 2, dtype=torch.float32, device=lab.device)
    _lib.check(_lib.lib().pea_label_weights(ctypes.byref(d), _ptr(lab), flags, _ptr(wtab), _ptr(counts), cb, _stream()),
               "pea_label_weights")
    return wtab, counts, cb


def label_counts(d, dev):
    """-> (counts, cb): the scratch of the label count reductions (pea_label_weights, pea_gen_targets) and its size in bytes"""
    cb = _lib.lib().pea_targets_workspace_bytes(ctypes.byref(d))
    return torch.empty(max(cb, 4) // 4, dtype=torch.int32, device=dev), cb


def check_weight_table(wtab, j, B, K, dev):
    """a caller's weight table for loss j must be what label_weight_table makes for this batch and stencil -> wtab"""
    if wtab.numel() != B * K * 2 or wtab.dtype != torch.float32 or wtab.device != dev:
        raise ValueError("weight table %d does not fit this batch / stencil" % j)
    if not wtab.is_contiguous():
        raise ValueError("weight table %d must be contiguous" % j)
    return wtab


_MULTI_LABELS_OK = _IdMemo(256)


def multi_labels_call(specs, e_cs, sources, flags, tables, need_affs, rows, dlosses):
    """ONE pea_affinity_fwd_bwd_labels_multi call (include/pea_multi_labels.h): loss rows into `rows`, de_j = dlosses[j] (device
    scalars, or None = 1) * d loss_j / d e_j -> (affs list, de list; de_j in the dtype of e_j: float32 / float16 / bfloat16, one for
    the whole table).  Raises MultiLabelsUnsupported before anything is launched."""
    n = len(e_cs)
    L = _lib.lib()
    dev = e_cs[0].device
    if not 1 <= n <= _lib.PEA_MULTI_MAX_N:
        raise MultiLabelsUnsupported("at most %d losses per call" % _lib.PEA_MULTI_MAX_N)
    descs, labs, conv = [], [], {}
    for spec, e_c, (lab, step) in zip(specs, e_cs, sources):
        if e_c.device != dev or lab.device != dev:
            raise RuntimeError("all operands must live on %s" % dev)
        if not labels_offsets_in_range(spec, e_c):
            raise MultiLabelsUnsupported("an offset is as long as the image (see labels_offsets_in_range)")
        descs.append(make_desc(spec, e_c))
        if id(lab) not in conv:  # (one tensor sampled by every entry is converted and range-checked once)
            conv[id(lab)] = _labels_int32(lab)
        labs.append(conv[id(lab)])
    table = (_lib.PeaMultiLabels * n)()
    for j in range(n):
        a, lab, step = table[j], labs[j], sources[j][1]
        a.desc, a.e, a.labels = ctypes.pointer(descs[j]), e_cs[j].data_ptr(), lab.data_ptr()
        a.label_dims[:] = [1] * (4 - lab.dim()) + list(lab.shape[1:])
        a.label_step[:] = step
    geometry = tuple(tuple(a.label_dims) + tuple(a.label_step) for a in table) + (flags,)
    if not _MULTI_LABELS_OK.get(tuple(descs), geometry, lambda: bool(L.pea_multi_labels_supported(table, n, flags))):
        raise MultiLabelsUnsupported("the table is outside the fused set of include/pea_multi_labels.h")
    with _on_device(dev):
        affs = [torch.empty(_affs_shape(e_c, sp.K) if need_affs else (0,), dtype=torch.float32, device=dev) for e_c, sp in zip(e_cs, specs)]
        des = [torch.empty_like(e_c) for e_c in e_cs]
        for j in range(n):
            a = table[j]
            if tables is not None and tables[j] is not None:
                a.wtab = check_weight_table(tables[j], j, e_cs[j].shape[0], specs[j].K, dev).data_ptr()
            a.affs = affs[j].data_ptr() if need_affs else None
            a.loss_out, a.de = rows[j].data_ptr(), des[j].data_ptr()
            a.dloss = None if dlosses is None or dlosses[j] is None else dlosses[j].data_ptr()
        sb = int(L.pea_multi_labels_scratch_bytes(table, n))
        scratch = torch.empty(max(sb, 4) // 4, dtype=torch.int32, device=dev)
        work, wsb = workspace(dev, descs[0], n)
        rc = L.pea_affinity_fwd_bwd_labels_multi(table, n, flags, _ptr(work), wsb, _ptr(scratch), sb, _stream())
    if rc == _lib.E_UNSUPPORTED:  # (nothing was launched)
        raise MultiLabelsUnsupported("pea_affinity_fwd_bwd_labels_multi: the table is outside the fused set")
    _lib.check(rc, "pea_affinity_fwd_bwd_labels_multi")
    return affs, des


class MultiLabelsAffinityMSE(torch.autograd.Function):
    """n self losses straight from label images as ONE node and ONE library call (include/pea_multi_labels.h): a count launch for the
    class-balance tables, one fused forward + backward launch over every tile of every scale, one loss finish.

        loss_0 .., affs_0 .., per_offset_0 .. = f(specs, sources, flags, need_affs, tables, *embeddings)

    specs: n AffinitySpecs; sources: label_sources(...) -- per loss (label tensor, (sz, sy, sx)), a tensor of its own or one all
    losses sample with a step; flags: _lib.TGT_*; tables: None or per loss None / a [B, K, 2] table of pea_label_weights.
    The gradients are computed for grad_output = 1 and backward() hands them out scaled by autograd's grad_outputs; a caller that
    owns the weighting and the backward (the section node) calls multi_labels_call itself.  Raises MultiLabelsUnsupported before
    anything is launched."""

    @staticmethod
    def forward(ctx, specs, sources, flags, need_affs, tables, *embs):
        ctx.set_materialize_grads(False)
        n = len(embs)
        if not (len(specs) == len(sources) == n):
            raise ValueError("one spec and one label source per embedding")
        e_cs = [_embedding_arg(e, "embedding") for e in embs]
        dev = e_cs[0].device
        with _on_device(dev):
            rows = _loss_rows(specs, dev).unbind(0)
            affs, ctx.des = multi_labels_call(specs, e_cs, sources, flags, tables, need_affs, rows, None)
            ctx.args = (specs, [st for _, st in sources], flags)
            ctx.n_tab = 0 if tables is None else n
            tabs = [] if tables is None else [t if t is not None else torch.empty(0, device=dev) for t in tables]
            ctx.save_for_backward(*(e_cs + [lab for lab, _ in sources] + tabs))
        ctx.n = n
        losses = [rows[j][0] for j in range(n)]
        parts = [rows[j][1:1 + specs[j].K] for j in range(n)]
        ctx.mark_non_differentiable(*(affs + parts))
        return tuple(losses) + tuple(affs) + tuple(parts)

    @staticmethod
    def backward(ctx, *grads):
        n = ctx.n
        live = [j for j in range(n) if grads[j] is not None and ctx.needs_input_grad[5 + j]]
        if not live:
            return (None,) * (5 + n)
        if ctx.des is None:  # a second backward over a retained graph: the call once more on the saved inputs
            saved = ctx.saved_tensors
            specs, steps, flags = ctx.args
            e_cs, labs = list(saved[:n]), saved[n:2 * n]
            tables = [t if t.numel() else None for t in saved[2 * n:]] if ctx.n_tab else None
            with _on_device(e_cs[0].device):
                rows = _loss_rows(specs, e_cs[0].device).unbind(0)
                _, ctx.des = multi_labels_call(specs, e_cs, list(zip(labs, steps)), flags, tables, False, rows, None)
        des, ctx.des = ctx.des, None
        out = [None] * n
        with _on_device(des[0].device):
            for j in live:  # (the buffers were written for grad_output = 1: rescaled in place, untouched where that is exactly 1)
                de = des[j]
                dl = grads[j].to(device=de.device, dtype=torch.float32).contiguous()
                # (a 16-bit de was rounded when it was stored: a grad_output that is no power of two rounds it a second time, as
                #  LabelsAffinityMSE does -- within one ulp of the f32 product rounded once, tests/test_gpu_multi16.py)
                _lib.check(_lib.lib().pea_scale_inplace(_ptr(de), _DTYPE_CODE[de.dtype], de.numel(), _ptr(dl), _stream()),
                           "pea_scale_inplace")
                out[j] = de
        return (None,) * 5 + tuple(out)


class LabelsAffinityMSE(torch.autograd.Function):
    """loss, affs, per_offset_losses = f(e, e_other, labels): the training step straight from the label image
    (pea_label_weights + pea_affinity_fwd_bwd_labels): target / mask / weight are evaluated inside the kernel and
    d loss / d e comes out of the same launch (for grad_output = 1; backward() rescales it in place).
    flags: _lib.TGT_* (2D reference path: PADDING | MASK_INSIDE; 3D: BOTH_FOREGROUND)."""

    @staticmethod
    def forward(ctx, e, e_other, labels, spec, flags, need_affs=True):
        ctx.set_materialize_grads(False)
        e_c, o_c = _pair_args(e, e_other)
        _require_gpu(labels, "labels")
        if labels.dtype.is_floating_point or tuple(labels.shape) != (e_c.shape[0],) + tuple(e_c.shape[2:]):
            raise ValueError("labels must be an integer tensor of shape %s" % ((e_c.shape[0],) + tuple(e_c.shape[2:]),))
        lab = _labels_int32(labels)
        if not labels_offsets_in_range(spec, e_c):
            raise LabelsStepUnsupported("an offset is as long as the image: the labels-in kernels would fold it (torch.roll) where "
                                        "gen_affs_ours masks it out; use gen_targets + the tensor API")
        kshape = _affs_shape(e_c, spec.K)
        with _on_device(e_c.device):
            d = make_desc(spec, e_c)
            L = _lib.lib()
            affs = torch.empty(kshape if need_affs else (0,), dtype=torch.float32, device=e_c.device)
            loss_vec = torch.empty(1 + spec.K, dtype=torch.float32, device=e_c.device)
            wtab, _, _ = label_weight_table(d, lab, flags, e_c.shape[0], spec.K)
            work, wsb = workspace(e_c.device, d)
            de_unit = torch.empty_like(e_c)
            # large self losses on the cross kernels: two launches (labels-in forward + cross backward) through a scratch buffer
            # for g and the 1 / norm plane; small ones are launch-bound and keep the one-launch kernel
            scratch, sb = None, 0
            if o_c is None and e_c.numel() // e_c.shape[1] >= LABELS_TWO_LAUNCH_MIN_PX:
                sb = int(L.pea_labels_scratch_bytes(ctypes.byref(d)))
                if sb:
                    scratch = torch.empty(sb // 4, dtype=torch.float32, device=e_c.device)
            rc = L.pea_affinity_fwd_bwd_labels_ex(ctypes.byref(d), _ptr(e_c), _ptr(o_c), _ptr(lab), _ptr(wtab), flags,
                                                  _ptr(affs) if need_affs else None, _ptr(loss_vec), None, _ptr(de_unit), _ptr(work), wsb,
                                                  _ptr(scratch), sb, _stream())
            if rc == _lib.E_UNSUPPORTED:
                raise LabelsStepUnsupported("no labels-in kernel for this descriptor (D != 16, image smaller than a tile, "
                                            "stencil too wide): use gen_targets + the tensor API")
            _lib.check(rc, "pea_affinity_fwd_bwd_labels")
        ctx.de_unit, ctx.desc = de_unit, d
        # for a second backward over a retained graph: saved like inputs (freed after a non-retained backward, version-checked on a
        # retained one), nothing is copied
        ctx.save_for_backward(e_c, o_c, lab, wtab)
        ctx.lflags = flags
        loss, per_offset = loss_vec[0], loss_vec[1:]
        ctx.mark_non_differentiable(affs, per_offset)
        return loss, affs, per_offset

    @staticmethod
    def _unit_gradient_again(ctx):
        """the gradient for grad_output = 1 once more (the first backward handed its buffer over, scaled in place): the step is run
        again on the saved inputs -- a retained graph is the rare case, and keeping a pristine copy would cost every step 150 MB"""
        e_c, o_c, lab, wtab = ctx.saved_tensors
        flags = ctx.lflags
        d, L = ctx.desc, _lib.lib()
        with _on_device(e_c.device):
            loss_vec = torch.empty(1 + d.K, dtype=torch.float32, device=e_c.device)
            work, wsb = workspace(e_c.device, d)
            de_unit = torch.empty_like(e_c)
            _lib.check(L.pea_affinity_fwd_bwd_labels_ex(ctypes.byref(d), _ptr(e_c), _ptr(o_c), _ptr(lab), _ptr(wtab), flags, None,
                                                        _ptr(loss_vec), None, _ptr(de_unit), _ptr(work), wsb, None, 0, _stream()),
                       "pea_affinity_fwd_bwd_labels")
        return de_unit

    @staticmethod
    def backward(ctx, dloss, _daffs, _dvec):
        if not ctx.needs_input_grad[0] or dloss is None:
            return None, None, None, None, None, None
        if ctx.de_unit is None:  # a second backward over a retained graph
            ctx.de_unit = LabelsAffinityMSE._unit_gradient_again(ctx)
        de, ctx.de_unit = ctx.de_unit, None
        with _on_device(de.device):
            dl = dloss.to(device=de.device, dtype=torch.float32).contiguous()
            _lib.check(_lib.lib().pea_scale_inplace(_ptr(de), ctx.desc.dtype, de.numel(), _ptr(dl), _stream()), "pea_scale_inplace")
        return de, None, None, None, None, None
