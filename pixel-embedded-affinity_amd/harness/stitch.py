"""3D inference stitcher on the device: Provider_valid.reset_output / get_weight / add_vol / get_results of
scripts_ac3ac4/data/provider_valid.py:291-349 (model_type 'superhuman') without the per-window D2H copy and numpy
accumulation (scripts_ac3ac4/inference.py:166, main.py:302).  The Gaussian blend weights are computed exactly as the
reference does (numpy, float32 linspace / meshgrid) once on the host; everything per window runs in pea_stitch_add -- or, from the
embedding itself, in pea_affinity_infer_stitch (add_embedding: affinities, border fill, relu and blend in one launch per window).
"""
import ctypes

import numpy as np
import torch

from .. import _lib
from ..affinity_op import AffinitySpec, _embedding_arg, _on_device, _ptr, _stream, affinity_infer, make_desc
from ..utils.affinity_ours import NORM5_SHIFTS, axis_offsets_3d
from ..utils.postproc import fill_border_relu_


def get_weight(out_size, sigma=0.2, mu=0.0):
    """provider_valid.py:305-318 (num_z >= 18 branch): [1, oz, oy, ox] float32"""
    zz, yy, xx = np.meshgrid(np.linspace(-1, 1, out_size[0], dtype=np.float32),
                             np.linspace(-1, 1, out_size[1], dtype=np.float32),
                             np.linspace(-1, 1, out_size[2], dtype=np.float32), indexing='ij')
    dd = np.sqrt(zz * zz + yy * yy + xx * xx)
    weight = 1e-6 + np.exp(-((dd - mu) ** 2 / (2.0 * sigma ** 2)))
    return weight[np.newaxis, ...]


_SPECS = {}


def _mode_spec(embedding_mode):
    """the spec of inf_embedding_loss_norm1 / _norm5 (loss/loss_embedding_mse_3d.py), built once: a window costs tens of microseconds"""
    spec = _SPECS.get(embedding_mode)
    if spec is None:
        shifts = NORM5_SHIFTS if embedding_mode == 5 else (1, 1, 1)
        spec = _SPECS[embedding_mode] = AffinitySpec(3, axis_offsets_3d(shifts), None, _lib.BORDER_CROP_ZERO, _lib.NORM_CROPPED, 1e-12)
    return spec


def _with_relu(spec):
    """`spec` with PEA_FLAG_RELU_AFFS, remembered on the spec itself"""
    r = getattr(spec, "_relu_twin", None)
    if r is None or (r.offsets, r.lam, r.border, r.norm, r.eps, r.act) != (spec.offsets, spec.lam, spec.border, spec.norm, spec.eps,
                                                                            spec.act | _lib.FLAG_RELU_AFFS):
        r = spec._relu_twin = AffinitySpec(spec.ndim, spec.offsets, spec.lam, spec.border, spec.norm, spec.eps, True, spec.act)
    return r


class VolumeStitcher(object):
    """out_affs [C, Z, Y, X] / weight_map [1, Z, Y, X] on the GPU; windows of out_size = (oz, oy, ox)."""

    def __init__(self, channels, vol_shape, out_size, device, sigma=0.2, mu=0.0):
        self.C, self.shape, self.out_size = int(channels), tuple(int(v) for v in vol_shape), tuple(int(v) for v in out_size)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("VolumeStitcher runs on an MI355X only (no CPU fallback)")
        self.weight_vol = torch.from_numpy(np.ascontiguousarray(get_weight(self.out_size, sigma, mu), dtype=np.float32)).to(self.device)
        self.reset_output()

    def reset_output(self):
        """provider_valid.py:291-303"""
        self.out_affs = torch.zeros((self.C,) + self.shape, dtype=torch.float32, device=self.device)
        self.weight_map = torch.zeros((1,) + self.shape, dtype=torch.float32, device=self.device)

    def add_vol(self, affs_vol, pos):
        """provider_valid.py:320-331.  affs_vol [C, oz, oy, ox] (f32, on the GPU); pos = (z0, y0, x0) start of the window
        in the volume.  (The reference slices the 2nd spatial dim with `fromx` and the 3rd with `fromy`, :326-331; its
        windows are square in y/x, so pass pos = (fromz, fromx, fromy) to reproduce it literally.)"""
        if not affs_vol.is_cuda or affs_vol.dtype != torch.float32:
            raise ValueError("affs_vol must be a float32 tensor on the GPU")
        v = affs_vol.reshape((self.C,) + self.out_size).contiguous()
        Z, Y, X = self.shape
        oz, oy, ox = self.out_size
        p = lambda t: ctypes.c_void_p(t.data_ptr())
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().pea_stitch_add(p(self.out_affs), p(self.weight_map), p(v), p(self.weight_vol), self.C, Z, Y, X,
                                                 oz, oy, ox, int(pos[0]), int(pos[1]), int(pos[2]),
                                                 ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), "pea_stitch_add")

    def add_embedding(self, embedding, pos, embedding_mode=5, shift=1, relu=True, spec=None, fused=False):
        """scripts_ac3ac4/inference.py:150-166 from the embedding on: inf_embedding_loss_norm1 / _norm5 (embedding_mode 1 / 5; `spec`
        overrides it), the border fill of channels 0..2 by `shift` (:160-163; 0 = none), F.relu (:164) and add_vol (:166).
        embedding [B, D, oz, oy, ox] on the GPU, f32 / f16 / bf16; pos = one (z0, y0, x0) or B of them.  Batch items are issued as B
        calls in order (overlapping windows read-modify-write the same voxels: one launch never holds two).  fused=True: one launch
        per window (pea_affinity_infer_stitch) where the library fuses the descriptor; elsewhere, and with fused=False, the three
        calls affinity_infer, fill_border_relu_, add_vol.  fused=False is the default until profiles/infer_stitch_ab.py has shown
        the one-launch form faster on an MI355X."""
        e = _embedding_arg(embedding, "embedding").detach()
        if e.dim() != 5 or tuple(e.shape[2:]) != self.out_size:
            raise ValueError("embedding must be [B, D] + %s, got %s" % (self.out_size, tuple(e.shape)))
        if e.device != self.weight_vol.device:
            raise ValueError("embedding is on %s, the stitcher on %s" % (e.device, self.weight_vol.device))
        B = e.shape[0]
        pos = np.asarray(pos, dtype=np.int64)
        pos = np.broadcast_to(pos, (B, 3)) if pos.ndim == 1 else pos
        if pos.shape != (B, 3):
            raise ValueError("pos must be (z0, y0, x0) or one per batch item, got shape %s" % (pos.shape,))
        if spec is None:
            if embedding_mode not in (1, 5):
                raise NotImplementedError("embedding_mode must be 1 or 5 (or pass spec)")
            spec = _mode_spec(embedding_mode)
        if spec.K != self.C:
            raise ValueError("the spec has %d channels, the stitcher %d" % (spec.K, self.C))
        fspec = _with_relu(spec) if relu and not spec.relu else spec  # F.relu rides in the descriptor's activation bits
        L = _lib.lib()
        Z, Y, X = self.shape
        with _on_device(e.device):
            for b in range(B):
                eb = e[b:b + 1]
                d = make_desc(fspec, eb)
                if fused and L.pea_infer_stitch_supported(ctypes.byref(d), int(shift)):
                    _lib.check(L.pea_affinity_infer_stitch(ctypes.byref(d), _ptr(eb), int(shift), _ptr(self.weight_vol), _ptr(self.out_affs),
                                                           _ptr(self.weight_map), Z, Y, X, int(pos[b][0]), int(pos[b][1]), int(pos[b][2]),
                                                           _stream()), "pea_affinity_infer_stitch")
                else:
                    pred = fill_border_relu_(affinity_infer(eb, None, spec), shift=shift, relu=relu)
                    self.add_vol(pred[0], pos[b])

    def add_distance_embedding(self, embedding, pos, offsets, delta_v, delta_d, border, invert=False):
        """A window of a model trained with the discriminative loss: the distance-form affinities of the raw embedding
        (harness/dist.py distance_affinities, include/pea_dist.h) followed by add_vol -- two launches per window.
        embedding [B, D, oz, oy, ox] on the GPU, f32 / f16 / bf16; pos = one (z0, y0, x0) or B of them; len(offsets) channels.  Batch
        items are added in order, as add_embedding does."""
        from .dist import distance_affinities
        if not isinstance(embedding, torch.Tensor) or embedding.dim() != 5 or tuple(embedding.shape[2:]) != self.out_size:
            raise ValueError("embedding must be [B, D] + %s, got %s" % (self.out_size, tuple(getattr(embedding, "shape", ()))))
        if len(offsets) != self.C:
            raise ValueError("%d offsets, the stitcher has %d channels" % (len(offsets), self.C))
        B = embedding.shape[0]
        pos = np.asarray(pos, dtype=np.int64)
        pos = np.broadcast_to(pos, (B, 3)) if pos.ndim == 1 else pos
        if pos.shape != (B, 3):
            raise ValueError("pos must be (z0, y0, x0) or one per batch item, got shape %s" % (pos.shape,))
        affs = distance_affinities(embedding.detach(), offsets, delta_v=delta_v, delta_d=delta_d, border=border, invert=invert)
        if affs.device != self.weight_vol.device:
            raise ValueError("embedding is on %s, the stitcher on %s" % (affs.device, self.weight_vol.device))
        for b in range(B):
            self.add_vol(affs[b], pos[b])

    def get_results(self, valid_padding):
        """provider_valid.py:337-349: out / weight_map, cropped by valid_padding (a view of the device tensor)"""
        Z, Y, X = self.shape
        p = lambda t: ctypes.c_void_p(t.data_ptr())
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().pea_stitch_finalize(p(self.out_affs), p(self.weight_map), self.C, Z * Y * X,
                                                      ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), "pea_stitch_finalize")
        return self._cropped(valid_padding)

    def _cropped(self, valid_padding):
        """the view get_results returns: out_affs cropped by valid_padding (provider_valid.py:341-348)"""
        vz, vy, vx = (int(v) for v in valid_padding)
        out = self.out_affs
        if vz:
            out = out[:, vz:-vz]
        return out[:, :, vy:-vy, vx:-vx] if (vy and vx) else out

    def finish(self, valid_padding, gt_affs, channels=3, clip=(1e-6, 0.999999)):
        """get_results AND the three scalars scripts_ac3ac4/main.py:339-351 logs on every save (whole_mse, whole_bce, whole_f1 of
        out_affs[:channels] against gt_affs) in ONE data launch (pea_affs_metrics with DIVIDE | STORE, include/pea_metrics.h): the
        division by the weight map is written back to the whole volume -- the bits of get_results -- while the first `channels`
        channels of the cropped region are compared with gt_affs [channels, Z', Y', X'] (float32, on the GPU).  clip: the bounds of
        np.clip at :345.  Returns (out, metrics): the view get_results returns and an AffinityMetrics; nothing is copied to the host."""
        from .metrics import affinity_metrics
        if not isinstance(gt_affs, torch.Tensor) or not gt_affs.is_cuda:
            raise RuntimeError("VolumeStitcher.finish runs on an MI355X only (no CPU fallback): gt_affs must be a device tensor")
        out = self._cropped(valid_padding)
        if gt_affs.dim() != 4 or tuple(gt_affs.shape) != (int(channels),) + tuple(out.shape[1:]):
            raise ValueError("gt_affs must be %s, got %s" % ((int(channels),) + tuple(out.shape[1:]), tuple(gt_affs.shape)))
        vz, vy, vx = (int(v) for v in valid_padding)
        origin = (vz, vy, vx) if (vy and vx) else (vz, 0, 0)
        metrics = affinity_metrics(self.out_affs.unsqueeze(0), gt_affs.unsqueeze(0), None, store=True, weight_map=self.weight_map,
                                   clip=(np.float32(clip[0]), np.float32(clip[1])), origin=origin, channels=int(channels))
        return out, metrics
