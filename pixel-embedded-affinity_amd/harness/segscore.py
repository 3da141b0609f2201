"""The segmentation scores of the validation loops on the device (include/pea_segscore.h: pea_seg_scores): what the reference's
drivers compute per validation image or volume,

  scripts_cvppp/main.py:413-417 (scripts_bbbc039v1/main.py likewise)   SymmetricBestDice, AbsDiffFGLabels (utils/evaluate.py),
                                                                       skimage's adapted_rand_error and variation_of_information
  scripts_ac3ac4/main.py:322-327, inference.py:199-244                 VOI and ARAND, once for waterz and once for LMC

from ONE contingency table of the predicted against the ground-truth label image: one streaming launch over the pixels, three over the
table's slots, one small finish.  No host synchronisation for labels of up to 32 bits (the call can be captured with pea.graphed);
every column is bit-reproducible (integer sums).  utils/evaluate.py and utils/seg_scores.py carry the reference's names and signatures.
"""
import ctypes

import numpy as np
import torch

from .. import _lib
from ..affinity_op import _on_device, _ptr, _stream, stream_workspace

CAPACITY_FLOOR, CAPACITY_CAP = 256, 32768  # of the default capacity (default_capacity)
_NARROW = (torch.uint8, torch.int8, torch.int16, torch.uint16, torch.int32)
_WIDE = (torch.int64, torch.uint64)
_NP_OK = (np.uint8, np.int8, np.int16, np.uint16, np.int32, np.int64, np.uint64)


def default_capacity(S, ceiling=CAPACITY_CAP):
    """slots per image when the caller names none: the power of two at or above S / 32, at least 256 and at most 32768 (one slot
    per 32 pixels covers the drivers' images many times over: a 544 x 544 CVPPP image has some 100 pairs and gets 16384 slots, a
    1024 x 1024 image with several thousand ids gets 32768; 80 bytes per slot and image).  A table that turns out too small is
    retried once at four times the size when the scores are read (SegmentationScores)."""
    want = max(1, (int(S) + 31) // 32)
    cap = 1 << (want - 1).bit_length()
    return min(ceiling, max(CAPACITY_FLOOR, cap))


def _workspace(dev, nb):
    """the tables of pea_seg_scores / pea_seg_table for the CURRENT stream of `dev` (every call leaves them all zero but for the magic
    word: ready for ANY descriptor that fits)"""
    return stream_workspace("seg", dev, nb, _lib.lib().pea_seg_workspace_init, "pea_seg_workspace_init")


def labels_int32(x, name="labels", device=None):
    """a label image as the kernels take it: a contiguous int32 tensor, on `device` if one is named (numpy arrays and CPU tensors --
    the segmentation comes from elf or waterz on the host -- are narrowed on the host and then uploaded).
    uint8 / int8 / int16 / uint16 / int32 are widened as they are.  int64 / uint64 are narrowed after ONE range check, which for a
    device tensor is one host synchronisation (for these two dtypes only); a value above 2^31 - 1 or below -2^31 raises ValueError.
    Negative values that fit are passed on: the kernels count them (n_bad)."""
    if isinstance(x, np.ndarray):
        if x.dtype.type not in _NP_OK:
            raise TypeError("%s must hold integer ids (uint8, int16, uint16, int32, int64 or uint64), got %s" % (name, x.dtype))
        if x.dtype in (np.int64, np.uint64):
            if x.size and (int(x.max()) > 2 ** 31 - 1 or int(x.min()) < -2 ** 31):
                raise ValueError("%s holds ids outside int32 (%d .. %d): relabel the segmentation first" % (name, int(x.min()), int(x.max())))
        t = torch.from_numpy(np.ascontiguousarray(x.astype(np.int32, copy=False)))
    elif isinstance(x, torch.Tensor):
        t = x.detach()
        if t.dtype in _WIDE:
            if t.numel():
                if t.dtype == torch.uint64:  # ids >= 2^63 come out negative and are refused like any value below -2^31
                    t = t.view(torch.int64)
                    lo, hi = (int(v) for v in torch.aminmax(t))
                    lo = lo if lo >= 0 else -2 ** 63
                else:
                    lo, hi = (int(v) for v in torch.aminmax(t))
                if hi > 2 ** 31 - 1 or lo < -2 ** 31:
                    raise ValueError("%s holds ids outside int32 (%d .. %d): relabel the segmentation first" % (name, lo, hi))
            t = t.to(torch.int32)
        elif t.dtype in _NARROW:
            t = t if t.dtype == torch.int32 else t.to(torch.int32)
        else:
            raise TypeError("%s must hold integer ids (uint8, int16, uint16, int32, int64 or uint64), got %s" % (name, t.dtype))
    else:
        raise TypeError("%s must be a numpy array or a torch.Tensor, got %s" % (name, type(x).__name__))
    if device is not None and t.device != device:
        t = t.to(device)
    return t if t.is_contiguous() else t.contiguous()


def _args(pred, gt, batched):
    """-> (pred, gt) as int32 [B, S] on one GPU: shapes and dtypes first, then the device, so that what is wrong with a call can be
    said without a GPU"""
    for x, name in ((pred, "pred"), (gt, "gt")):
        if not isinstance(x, (np.ndarray, torch.Tensor)):
            raise TypeError("%s must be a numpy array or a torch.Tensor, got %s" % (name, type(x).__name__))
    if tuple(pred.shape) != tuple(gt.shape):
        raise ValueError("pred %s and gt %s differ in shape" % (tuple(pred.shape), tuple(gt.shape)))
    if len(pred.shape) == 0 or int(np.prod(pred.shape)) == 0:
        raise ValueError("pred is empty: %s" % (tuple(pred.shape),))
    dev = None
    for x in (pred, gt):
        if isinstance(x, torch.Tensor) and x.is_cuda:
            if dev is not None and x.device != dev:
                raise RuntimeError("pred is on %s, gt on %s" % (pred.device, gt.device))
            dev = x.device
    P, G = labels_int32(pred, "pred"), labels_int32(gt, "gt")
    if dev is None:
        if not torch.cuda.is_available():
            raise RuntimeError("segmentation_scores runs on an MI355X only (no CPU fallback), and no GPU is visible")
        dev = torch.device("cuda", torch.cuda.current_device())
    B = int(P.shape[0]) if batched else 1
    return P.to(dev).reshape(B, -1), G.to(dev).reshape(B, -1)


def _launch(P, G, capacity):
    d = _lib.PeaSegDesc()
    d.B, d.S, d.capacity, d.flags = int(P.shape[0]), int(P.shape[1]), int(capacity), 0
    L = _lib.lib()
    rc = L.pea_seg_validate(ctypes.byref(d))
    if rc:
        raise ValueError("invalid segmentation-score descriptor (%s): B=%d, S=%d, capacity=%d (a power of two >= %d)"
                         % (L.pea_strerror(rc).decode(), d.B, d.S, d.capacity, _lib.SEG_MIN_CAPACITY))
    dev = P.device
    with _on_device(dev):
        out = torch.empty((d.B, _lib.SEG_COLS), dtype=torch.float64, device=dev)
        nb = int(L.pea_seg_workspace_bytes(ctypes.byref(d)))
        work = _workspace(dev, nb)
        _lib.check(L.pea_seg_scores(ctypes.byref(d), _ptr(P), _ptr(G), _ptr(out), _ptr(work), nb, _stream()), "pea_seg_scores")
    return out, d


class _ScoreTable(object):
    """A device score table [B, columns] whose column 0 is n_overflow, read lazily: the first read copies it to the host and, where a
    pair table overflowed, repeats the launch ONCE at four times the capacity.  A subclass names its COLUMNS and its _relaunch."""
    COLUMNS = ()

    def _relaunch(self, capacity):
        """launch again with `capacity`; sets self.table (and what else the launch returns)"""
        raise NotImplementedError

    def _rows(self):
        if self._host is None:
            host = self.table.detach().cpu().numpy()
            if (host[:, 0] != 0).any():
                first = self.capacity
                self._relaunch(4 * first)
                self.capacity = 4 * first
                host = self.table.detach().cpu().numpy()
                if (host[:, 0] != 0).any():
                    raise RuntimeError("the pair table overflowed at capacity %d and at %d (n_overflow %s): pass a larger capacity"
                                       % (first, self.capacity, host[:, 0].tolist()))
            self._host = host
        return self._host

    def _col(self, name, conv=float):
        c = self._rows()[:, self.COLUMNS.index(name)]
        vals = [conv(v) if np.isfinite(v) else float(v) for v in c]
        return vals[0] if len(vals) == 1 else vals


class SegmentationScores(_ScoreTable):
    """The device table [B, 19] (float64; columns _lib.SEG_COLUMNS) of one segmentation_scores call.  Nothing is copied to the host
    until a value is asked for.  The properties give a Python number for a single image and a list over the batch otherwise:
    .sbd / .best_dice / .best_dice_rev / .diff_fg / .abs_diff_fg / .fgbg_dice / .voi_split / .voi_merge / .voi (their sum) / .are /
    .are_precision / .are_recall / .n_overflow / .n_bad; .table is the device tensor, .contingency(b) the (pred id, gt id, count)
    triples of image b.

    If the first read finds n_overflow != 0 (the table was too small for the image's pairs), the call is repeated ONCE with four times
    the capacity; if that overflows too, RuntimeError."""

    COLUMNS = _lib.SEG_COLUMNS

    def __init__(self, table, pred, gt, capacity):
        self.table, self.capacity = table, int(capacity)
        self._pred, self._gt = pred, gt
        self._host = None

    def _relaunch(self, capacity):
        self.table, _ = _launch(self._pred, self._gt, capacity)

    sbd = property(lambda self: self._col("sbd"))
    best_dice = property(lambda self: self._col("best_dice"))
    best_dice_rev = property(lambda self: self._col("best_dice_rev"))
    diff_fg = property(lambda self: self._col("diff_fg", int))
    fgbg_dice = property(lambda self: self._col("fgbg_dice"))
    voi_split = property(lambda self: self._col("voi_split"))
    voi_merge = property(lambda self: self._col("voi_merge"))
    are = property(lambda self: self._col("are"))
    are_precision = property(lambda self: self._col("are_precision"))
    are_recall = property(lambda self: self._col("are_recall"))
    n_overflow = property(lambda self: self._col("n_overflow", int))
    n_bad = property(lambda self: self._col("n_bad", int))

    @property
    def abs_diff_fg(self):
        d = self.diff_fg
        return [abs(v) for v in d] if isinstance(d, list) else abs(d)

    @property
    def voi(self):
        s, m = self.voi_split, self.voi_merge
        return [a + b for a, b in zip(s, m)] if isinstance(s, list) else s + m

    def contingency(self, b=0):
        """-> (pred_ids int32 [n], gt_ids int32 [n], counts int64 [n]): the non-empty cells of image b's contingency table, sorted by
        (pred id, gt id) on the host (pea_seg_table: one more pass over image b, then one copy)"""
        B = int(self._pred.shape[0])
        if not 0 <= int(b) < B:
            raise IndexError("image %r of a batch of %d" % (b, B))
        self._rows()  # (settles the capacity)
        L = _lib.lib()
        d = _lib.PeaSegDesc()
        d.B, d.S, d.capacity, d.flags = B, int(self._pred.shape[1]), self.capacity, 0
        dev = self._pred.device
        n_max = int(min(self.capacity, d.S))
        with _on_device(dev):
            ids = torch.empty((2, n_max), dtype=torch.int32, device=dev)
            counts = torch.empty(n_max, dtype=torch.int64, device=dev)
            n_out = torch.empty(3, dtype=torch.int64, device=dev)
            nb = int(L.pea_seg_workspace_bytes(ctypes.byref(d)))
            work = _workspace(dev, nb)
            _lib.check(L.pea_seg_table(ctypes.byref(d), _ptr(self._pred), _ptr(self._gt), int(b), _ptr(ids[0]), _ptr(ids[1]), _ptr(counts),
                                       _ptr(n_out), n_max, _ptr(work), nb, _stream()), "pea_seg_table")
        n, dropped, _bad = (int(v) for v in n_out.cpu())
        if dropped:
            raise RuntimeError("the pair table overflowed at capacity %d (%d pixels dropped): pass a larger capacity" % (self.capacity, dropped))
        p, g, c = ids[0, :n].cpu().numpy(), ids[1, :n].cpu().numpy(), counts[:n].cpu().numpy()
        order = np.lexsort((g, p))
        return p[order], g[order], c[order]

    def __repr__(self):
        return "SegmentationScores(sbd=%s, voi=%s, are=%s)" % (self.sbd, self.voi, self.are)


def segmentation_scores(pred, gt, *, capacity=None, batched=None):
    """SBD, |DiffFGLabels|, FG/BG Dice, VOI and ARAND of a predicted against a ground-truth label image -> SegmentationScores.

    pred, gt   label images of one shape: a device tensor is used as it is, a numpy array or CPU tensor is uploaded.  uint8, int16,
               uint16 and int32 are taken as they are; int64 / uint64 are narrowed after one range check (labels_int32: one host
               synchronisation for a device tensor of these dtypes; ValueError above 2^31 - 1).  Negative ids are counted in
               n_bad and make that image's scores NaN.  Background is the lowest label for the Dice scores and label 0 of gt for
               VOI / ARAND (the reference's ignore_labels=(0)).
    batched    True: the first dimension counts images, each scored on its own ([B, ...]); False: one image of any shape ([...]).
               None (default): batched where there are more than two dimensions ([B, Y, X] is a batch, [Y, X] one image; pass
               batched=False for a single 3D volume).
    capacity   slots per image of the pair table, a power of two >= 64; None: default_capacity(S)"""
    if batched is None:
        batched = len(getattr(pred, "shape", ())) > 2
    P, G = _args(pred, gt, bool(batched))
    cap = default_capacity(P.shape[1]) if capacity is None else int(capacity)
    out, _ = _launch(P, G, cap)
    return SegmentationScores(out, P, G, cap)
