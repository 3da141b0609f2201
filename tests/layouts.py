"""The table of tensor layouts the Python entry points are held to (a helper module, no tests here; CPU or GPU tensors alike).

Every builder returns a VIEW with the requested shape whose values come from seeded dense data; `dense(view)` is its twin, the same
values in a fresh contiguous tensor.  The contract the tests check is "the call on the view equals the call on the twin".

  L1a / L1b  expanded over the batch from [...] / from [1, ...]            stride(0) == 0
  L2         expanded over dimension 1 (K, or the channel)                 stride(1) == 0
  L3         spatial crop of a larger tensor, big[..., 2:-2, 3:-1]
  L4         channel slice of a packed tensor, packed[:, K:2K]             dense items, batch stride 3 K S   (taken without a copy)
  L5         every other batch item, t[::2]                                dense items, batch stride 2 K S   (taken without a copy)
  L6         channels_last / channels_last_3d
  L7         an N...C tensor seen through permute(0, -1, 1, ...)
  L8         overlapping batch windows of one buffer (as_strided)          dense items, batch stride S < K S (read-only inputs)

L1 / L2 / L8 can be carved out of a tests/arena.py Arena with a trailing guard of (B - 1) * K * S elements: a reader that takes their
batch stride for the dense one then lands in the arena's NaN pattern, inside the allocation.
"""
import torch

VALUE_LAYOUTS = ("L1a", "L1b", "L2", "L3", "L4", "L5", "L6", "L7", "L8")
ZERO_COPY = ("L4", "L5", "L8")      # a dense [K, S] block per item at a positive batch stride
BROADCAST_BATCH = ("L1a", "L1b")


def numel(shape):
    n = 1
    for v in shape:
        n *= int(v)
    return n


def values(shape, dtype, seed, device="cpu"):
    """seeded dense data of `shape`: floats ~ N(0, 1) (float masks: uniform in [0, 1], fractional), integers / bool in {0, 1}"""
    g = torch.Generator().manual_seed(int(seed))
    if dtype == "mask_f32":
        t = torch.rand(tuple(shape), generator=g, dtype=torch.float32)
    elif dtype in (torch.float32, torch.float64):
        t = torch.randn(tuple(shape), generator=g, dtype=dtype)
    elif dtype in (torch.float16, torch.bfloat16):
        t = torch.randn(tuple(shape), generator=g, dtype=torch.float32).to(dtype)
    elif dtype == torch.bool:
        t = torch.randint(0, 2, tuple(shape), generator=g, dtype=torch.uint8).bool()
    else:
        t = torch.randint(0, 2, tuple(shape), generator=g, dtype=torch.int32).to(dtype)
    return t.to(device)


def dense(view):
    """the twin: the same values, freshly allocated and contiguous"""
    t = view.detach().clone(memory_format=torch.contiguous_format)
    assert t.is_contiguous() and torch.equal(t, view.detach())
    return t


def _place(src, arena, guard_elems, name):
    """`src` as it is, or copied to a view of `arena` followed by guard_elems elements (and the arena's usual 1 KiB) of its pattern"""
    if arena is None:
        return src, None
    v = arena.carve(tuple(src.shape), src.dtype, guard=1024 + guard_elems * src.element_size(), name=name)
    arena.fill(v, src)
    return v, v


def make(layout, shape, dtype, seed, device="cpu", arena=None, name=None):
    """-> (view of `shape`, the arena view behind it or None).  dtype: a torch dtype, or "mask_f32" (float32 in [0, 1])"""
    shape = tuple(int(v) for v in shape)
    B, K, sp = shape[0], shape[1], shape[2:]
    S = numel(sp)
    tdt = torch.float32 if dtype == "mask_f32" else dtype
    guard = B * K * S  # (more than the (B - 1) * K * S a dense-stride reader of a one-item source needs: enough for L2's [B, 1, S] too)
    if layout == "L1a":
        src, rec = _place(values((K,) + sp, dtype, seed, device), arena, guard, name)
        return src.expand(shape), rec
    if layout == "L1b":
        src, rec = _place(values((1, K) + sp, dtype, seed, device), arena, guard, name)
        return src.expand(shape), rec
    if layout == "L2":
        src, rec = _place(values((B, 1) + sp, dtype, seed, device), arena, guard, name)
        return src.expand(shape), rec
    if layout == "L3":
        big = values((B, K) + sp[:-2] + (sp[-2] + 4, sp[-1] + 4), dtype, seed, device)
        return big[..., 2:-2, 3:-1], None
    if layout == "L4":
        return values((B, 3 * K) + sp, dtype, seed, device)[:, K:2 * K], None
    if layout == "L5":
        return values((2 * B, K) + sp, dtype, seed, device)[::2], None
    if layout == "L6":
        fmt = torch.channels_last if len(sp) == 2 else torch.channels_last_3d
        return values(shape, dtype, seed, device).contiguous(memory_format=fmt), None
    if layout == "L7":
        nd = len(shape)
        return values((B,) + sp + (K,), dtype, seed, device).permute(0, nd - 1, *range(1, nd - 1)), None
    if layout == "L8":
        src, rec = _place(values(((B - 1) * S + K * S,), dtype, seed, device), arena, guard, name)
        strides, s = [], 1
        for v in reversed(sp):
            strides.insert(0, s)
            s *= v
        return torch.as_strided(src, shape, [S, S] + strides), rec
    if layout == "dense":
        return values(shape, dtype, seed, device), None
    raise ValueError(layout)


LABEL_LAYOUTS = ("L1a", "L1b", "L3", "L9s", "L9p", "L9n")


def label_values(shape, dtype, seed, device="cpu", n_ids=7, cell=5):
    """a blocky instance image of `shape` = (B, *spatial): ids 0 .. n_ids - 1 in cells of `cell` pixels in-plane (bool: id > 0)"""
    g = torch.Generator().manual_seed(int(seed))
    shape = tuple(int(v) for v in shape)
    coarse = shape[:-2] + (-(-shape[-2] // cell), -(-shape[-1] // cell))
    t = torch.randint(0, n_ids, coarse, generator=g, dtype=torch.int64)
    t = t.repeat_interleave(cell, -2).repeat_interleave(cell, -1)[..., :shape[-2], :shape[-1]]
    return (t > 0 if dtype == torch.bool else t.to(dtype)).to(device)


def make_labels(layout, B, sp, dtype, seed, device="cpu"):
    """a label view [B, *sp] ("L9n": [B, 1, *sp]):
      L1a / L1b  one image for the whole batch, expanded          L3   a crop of a larger image
      L9s        every other pixel in-plane, big[..., ::2, ::2]   L9p  plane 1 of a packed [B, 3, ...] tensor, packed[:, 1]
      L9n        the strided view of L9s with a channel axis of one, view[:, None]"""
    sp = tuple(int(v) for v in sp)
    if layout == "L1a":
        return label_values(sp, dtype, seed, device).expand((B,) + sp)
    if layout == "L1b":
        return label_values((1,) + sp, dtype, seed, device).expand((B,) + sp)
    if layout == "L3":
        return label_values((B,) + sp[:-2] + (sp[-2] + 4, sp[-1] + 4), dtype, seed, device)[..., 2:-2, 3:-1]
    if layout in ("L9s", "L9n"):
        v = label_values((B,) + sp[:-2] + (2 * sp[-2], 2 * sp[-1]), dtype, seed, device, cell=10)[..., ::2, ::2]
        return v if layout == "L9s" else v[:, None]
    if layout == "L9p":
        return label_values((B, 3) + sp, dtype, seed, device)[:, 1]
    if layout == "dense":
        return label_values((B,) + sp, dtype, seed, device)
    raise ValueError(layout)


def abi_view(out, bstride, shape):
    """what the C ABI reads of the tensor a normaliser returned: item b at data_ptr + b * (bstride or K * S) elements, a dense [K, S]
    block (include/pea.h) -- as a [B, K, S] tensor over the storage of `out`"""
    B, K = int(shape[0]), int(shape[1])
    S = numel(shape[2:])
    return torch.as_strided(out, (B, K, S), ((int(bstride) or K * S), S, 1))
