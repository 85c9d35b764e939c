"""A poisoned arena for footprint tests: where does a kernel read and write?

Every operand of a call is carved out of one flat uint8 buffer filled with a byte pattern that is a NaN in every
fp32 word (0x7FBFFFFF), a NaN in every fp16 half and a non-zero int8 code in every byte. A 2-D carve has a leading
dimension larger than its width, poisoned guard rows before and after it, poisoned pad columns [cols, ld) inside it
and a base that is `misalign`-byte aligned but not 2 * `misalign`-byte aligned. Each carve records which of its
bytes the callee may write (none for an input). After the inputs are filled, seal() snapshots the arena;
assert_untouched() then compares every byte outside the writable ranges with the snapshot and names the first
offender as (carve, row, column). An over-read shows in the result instead: it pulls NaN / garbage codes in.

Not a conftest: test modules import it as they import quant_backward_ref.
"""
import torch

POISON = (0xFF, 0xFF, 0xBF, 0x7F)   # little-endian fp32 0x7FBFFFFF (NaN); fp16 0xFFFF, 0x7FBF (NaN); int8 -1, -1, -65, 127
_GAP = 64                           # poisoned bytes between two carves


class Arena:
    def __init__(self, device, nbytes):
        self.nbytes = (int(nbytes) + 3) // 4 * 4
        raw = torch.empty(self.nbytes + 64, dtype=torch.uint8, device=device)
        skip = (-raw.data_ptr()) % 64           # offset 0 of the arena is 64-byte aligned
        self.buf = raw[skip:skip + self.nbytes]
        self.base = self.buf.data_ptr()
        self.buf.copy_(torch.tensor(POISON, dtype=torch.uint8).repeat(self.nbytes // 4).to(device))
        self.allowed = torch.zeros(self.nbytes, dtype=torch.bool, device=device)
        self.carves = []
        self.cursor = _GAP
        self.snapshot = None

    # ---- carving ---------------------------------------------------------------------------------
    def _place(self, lead_bytes, misalign, esize):
        assert misalign >= esize and misalign % esize == 0
        off = self.cursor + lead_bytes
        off += (misalign - (self.base + off)) % (2 * misalign)   # address = misalign (mod 2 misalign)
        return off

    def carve(self, rows, cols, ld, dtype, lead_rows=2, tail_rows=2, misalign=16, writable=None, name=None):
        """A [rows, cols] view with stride(0) == ld. writable: None (an input), True (columns [0, cols) of every
        row) or a column count w <= ld (columns [0, w) of every row, e.g. the zeroed code padding up to kpad)."""
        assert self.snapshot is None, "carve before seal()"
        assert rows >= 1 and 1 <= cols <= ld
        esize = torch.empty(0, dtype=dtype).element_size()
        pitch = ld * esize
        off = self._place(lead_rows * pitch, misalign, esize)
        end = off + (rows + tail_rows) * pitch
        assert end + _GAP <= self.nbytes, f"arena too small: {end + _GAP} > {self.nbytes}"
        self.cursor = end + _GAP
        wcols = 0 if writable is None else (cols if writable is True else int(writable))
        assert 0 <= wcols <= ld
        if wcols:
            torch.as_strided(self.allowed, (rows, wcols * esize), (pitch, 1), off).fill_(True)
        self.carves.append(dict(name=name or f"carve{len(self.carves)}", off=off, start=off - lead_rows * pitch, end=end,
                                rows=rows, cols=cols, pitch=pitch, esize=esize, wcols=wcols))
        view = self.buf[off:off + rows * pitch].view(dtype).view(rows, ld)[:, :cols]
        assert view.stride(0) == ld and view.data_ptr() % (2 * misalign) == misalign
        return view

    def carve_flat(self, n, dtype, misalign=16, writable=False, name=None):
        """n >= 1 contiguous elements with _GAP poisoned bytes on either side (elementwise operands, workspaces)."""
        return self.carve(1, n, n, dtype, lead_rows=0, tail_rows=0, misalign=misalign,
                          writable=True if writable else None, name=name)[0]

    def put(self, tensor, **kw):
        """An input carve ([rows, cols] with ld > cols, or flat for a 1-D tensor) holding `tensor`."""
        if tensor.dim() == 1:
            v = self.carve_flat(tensor.numel(), tensor.dtype, **kw)
        else:
            v = self.carve(tensor.shape[0], tensor.shape[1], kw.pop("ld"), tensor.dtype, **kw)
        v.copy_(tensor)
        return v

    def allow_bytes(self, view, offsets):
        """Marks bytes of the carve that `view` came from as writable: `offsets` are byte offsets from the view's
        first element (layouts whose writable set is not a column range, e.g. the rows < M of a tiled buffer)."""
        assert self.snapshot is None, "allow_bytes before seal()"
        start = view.data_ptr() - self.base
        c = next(c for c in self.carves if c["off"] == start)
        offsets = offsets.reshape(-1).to(self.allowed.device)
        assert int(offsets.min()) >= 0 and start + int(offsets.max()) < c["off"] + c["rows"] * c["pitch"]
        self.allowed[start + offsets] = True
        c["wcols"] = max(c["wcols"], 1)

    # ---- checking --------------------------------------------------------------------------------
    def seal(self):
        """Call once every input is filled and every in-place output holds its base values."""
        self.snapshot = self.buf.clone()

    def locate(self, off):
        for c in self.carves:
            if c["start"] <= off < c["end"]:
                row = (off - c["off"]) // c["pitch"]
                col = ((off - c["off"]) % c["pitch"]) // c["esize"]
                if row < 0:
                    kind = "lead guard row"
                elif row >= c["rows"]:
                    kind = "tail guard row"
                elif col >= c["cols"]:
                    kind = "pad column"
                else:
                    kind = "column outside the writable set" if c["wcols"] else "input"
                return c["name"], row, col, kind
        return "gap between carves", 0, off, "gap"

    def assert_untouched(self):
        assert self.snapshot is not None, "seal() the arena before the call"
        bad = (self.buf != self.snapshot) & ~self.allowed
        if bool(bad.any()):
            off = int(bad.nonzero()[0])
            name, row, col, kind = self.locate(off)
            raise AssertionError(f"{int(bad.sum())} bytes written outside the writable set; first at arena byte {off}: "
                                 f"{name} row {row} column {col} ({kind})")


# ---- operand helpers shared by the GPU footprint tests ----------------------------------------------------------
def scalar(v, dev):
    """A device float[1] (quantizer parameters and scales are passed as device scalars)."""
    return torch.tensor([float(v)], dtype=torch.float32, device=dev)


def round_up(v, m):
    return (v + m - 1) // m * m


def pack_codes(codes_w, wfmt, dev):
    """Packs integer weight codes exactly (linear quantizer with d = 1 and a large q_m, so code = w)."""
    from quantized_vit_amd import _lib
    n, k = codes_w.shape
    npad, kpad = round_up(n, _lib.TILE_N), round_up(k, _lib.TILE_K)
    ovf = torch.zeros(1, dtype=torch.int32, device=dev)
    packed = _lib.pack_weight(codes_w.float().to(dev).contiguous(), _lib.QT_LINEAR, scalar(1.0, dev), scalar(1000.0, dev),
                              None, wfmt, npad, kpad, ovf)
    torch.cuda.synchronize()
    assert ovf.item() == 0
    return packed, npad, kpad
