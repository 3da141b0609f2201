"""A guard-banded arena for tests that hand raw pointers to the C ABI (a plain helper, CPU or GPU tensors alike).

One uint8 buffer, base 256-byte aligned, filled with the 32-bit pattern 0x7fa5a5a5 (a NaN as f32; its upper half 0x7fa5 a NaN as
f16 and as bf16).  Views are carved out of it at a chosen address modulo 256 with untouched pattern bytes on both sides; a batch-strided
view also has pattern bytes between its batch items.  After the calls under test, check() asserts bit for bit that

  * every byte outside the views (guards, stride gaps) still holds the pattern,
  * every view that was only read still holds exactly what fill() put there,
  * no element of a view the kernel owns still holds the pattern: every element was written.

A 16-bit element is half a pattern word, and the lower half (0xa5a5) is an ordinary finite number that a kernel may well produce.
carve() therefore refills a 16-bit view with 0x7fa5 in EVERY element: each element is a NaN of its own and "still the pattern" is
unambiguous.  (u8 views cannot be `written` views for the same reason; no kernel here writes u8.)

The arena keeps a shadow copy of what every byte must be if nothing is written; the checks are comparisons with it through uint8 /
int32 views, so NaN payloads and signed zeros count.
"""
import torch

PATTERN = 0x7FA5A5A5
PATTERN16 = 0x7FA5
ALIGN = 256


class ArenaError(AssertionError):
    pass


class _Rec(object):
    def __init__(self, name, view, shadow, start, nbytes, item, batch, per, bstride):
        self.name, self.view, self.shadow, self.start, self.nbytes, self.item = name, view, shadow, start, nbytes, item
        self.batch, self.per, self.bstride = batch, per, bstride  # batch items of `per` elements, `bstride` elements apart


def _numel(shape):
    n = 1
    for v in shape:
        n *= int(v)
    return n


class Arena(object):
    def __init__(self, nbytes, device="cpu"):
        nbytes = (int(nbytes) + ALIGN - 1) // ALIGN * ALIGN
        self.device = torch.device(device)
        self._buf = torch.empty(nbytes + ALIGN, dtype=torch.uint8, device=self.device)
        off = (-self._buf.data_ptr()) % ALIGN
        self.raw = self._buf[off:off + nbytes]
        assert self.raw.data_ptr() % ALIGN == 0
        self.raw.view(torch.int32).fill_(PATTERN)
        self.expect = self.raw.clone()  # what every byte holds as long as nothing writes it
        self.nbytes, self.top, self.recs = nbytes, 0, []

    # ---- carving ---------------------------------------------------------------------------------------------------------------
    def _carve(self, shape, dtype, per, bstride, skew_bytes, guard, name):
        item = torch.empty((), dtype=dtype).element_size()
        if skew_bytes % item or not 0 <= skew_bytes < ALIGN:
            raise ValueError("skew_bytes must be a multiple of the element size below %d" % ALIGN)
        batch = int(shape[0]) if len(shape) else 1
        nel = (batch - 1) * bstride + per if batch else 0
        start = (self.top + guard + ALIGN - 1) // ALIGN * ALIGN + skew_bytes
        end = start + nel * item
        if end + guard > self.nbytes:
            raise ValueError("arena too small: %d bytes needed, %d there" % (end + guard, self.nbytes))
        self.top = end
        inner = [int(v) for v in shape[1:]]
        strides, s = [], 1
        for v in reversed(inner):
            strides.insert(0, s)
            s *= v
        strides = [bstride] + strides if len(shape) else []

        def typed(buf):
            flat = buf[start:end].view(dtype)
            return torch.as_strided(flat, [int(v) for v in shape], strides) if nel else flat.view([int(v) for v in shape])

        view, shadow = typed(self.raw), typed(self.expect)
        if item == 2 and nel:  # (module docstring) every 16-bit element a NaN of its own
            for v in (view, shadow):
                v.view(torch.int16).fill_(PATTERN16)
        rec = _Rec(name or "view%d" % len(self.recs), view, shadow, start, nel * item, item, batch, per, bstride)
        self.recs.append(rec)
        assert view.data_ptr() % ALIGN == skew_bytes
        return view

    def carve(self, shape, dtype, skew_bytes=0, guard=1024, name=None):
        """a contiguous view with data_ptr() % 256 == skew_bytes and >= guard pattern bytes before and after it"""
        n = _numel(shape)
        per = n // int(shape[0]) if len(shape) and int(shape[0]) else n
        return self._carve(tuple(shape), dtype, per, per, skew_bytes, guard, name)

    def carve_batch_strided(self, shape, dtype, extra_elems, skew_bytes=0, guard=1024, name=None):
        """the same with a batch stride of prod(shape[1:]) + extra_elems elements; the gap elements are guards too"""
        if extra_elems < 0 or len(shape) < 2:
            raise ValueError("a batch-strided view needs a batch dimension and extra_elems >= 0")
        per = _numel(shape[1:])
        return self._carve(tuple(shape), dtype, per, per + int(extra_elems), skew_bytes, guard, name)

    def _rec(self, view):
        for r in self.recs:
            if r.view is view or (r.view.data_ptr() == view.data_ptr() and r.view.shape == view.shape and r.view.dtype == view.dtype):
                return r
        raise ValueError("not a view of this arena")

    def fill(self, view, src):
        """copy data in (and remember it: an `untouched` view must still hold it at check())"""
        r = self._rec(view)
        src = torch.as_tensor(src).to(device=self.device, dtype=r.view.dtype)
        r.view.copy_(src)
        r.shadow.copy_(src)
        return view

    # ---- checking --------------------------------------------------------------------------------------------------------------
    def _owned_bytes(self, r):
        """bool [nbytes of the record]: the bytes of its elements (not of its stride gaps)"""
        el = torch.zeros((r.nbytes // r.item,), dtype=torch.bool, device=self.device)
        for b in range(r.batch):
            el[b * r.bstride:b * r.bstride + r.per] = True
        return el.repeat_interleave(r.item)

    def _where(self, off):
        prev = None
        for r in self.recs:
            if off < r.start:
                return "guard before '%s' (%d bytes before it)" % (r.name, r.start - off)
            if off < r.start + r.nbytes:
                rel = off - r.start
                el = rel // r.item
                if el % r.bstride >= r.per:
                    return "stride gap of '%s' (byte %d of the view's span)" % (r.name, rel)
                return "'%s' (byte %d of the view's span)" % (r.name, rel)
            prev = r
        return "guard after '%s' (%d bytes past it)" % (prev.name, off - prev.start - prev.nbytes) if prev else "the empty arena"

    def check(self, written=(), untouched=(), scratch=()):
        """scratch: views lent to the call with contents undefined before and after -- only their surroundings are checked"""
        wr = [self._rec(v) for v in written]
        sc = [self._rec(v) for v in scratch]
        for v in untouched:
            if self._rec(v) in wr or self._rec(v) in sc:
                raise ValueError("a view cannot be both written and untouched")
        diff = self.raw != self.expect
        for r in sc:
            diff[r.start:r.start + r.nbytes] &= ~self._owned_bytes(r)
        for r in wr:
            if r.item < 2:
                raise ValueError("a written view needs elements of 2 bytes or more")
            own = self._owned_bytes(r)
            seg = diff[r.start:r.start + r.nbytes]
            # an element none of whose bytes changed was not written
            same = (~seg.view(-1, r.item).any(dim=1)) & own.view(-1, r.item)[:, 0]
            if bool(same.any()):
                el = int(torch.nonzero(same)[0])
                raise ArenaError("unwritten element in '%s': byte offset %d of the view's span still holds the pattern (%d of %d elements)"
                                 % (r.name, el * r.item, int(same.sum()), r.batch * r.per))
            seg &= ~own  # (its own elements may differ; its stride gaps may not)
        if bool(diff.any()):
            off = int(torch.nonzero(diff)[0])
            raise ArenaError("byte %d of the arena changed: %s (%d bytes changed outside the written views)"
                             % (off, self._where(off), int(diff.sum())))
