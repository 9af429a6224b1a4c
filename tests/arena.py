"""Operands between poisoned borders: which memory may a kernel touch?

The value tests hand the library tensors straight from torch's caching allocator, so what lies before and after an operand is always
some other finite tensor.  A tap that reads row -1 and multiplies it by a zero flag, a 16-byte load that runs over the end of an odd
row, an epilogue that stores a whole tile where only a part exists: all of them give the right result there.  An ``Arena`` puts every
operand of a call into ONE uint8 buffer, as contiguous views at 512-byte offsets (the alignment the caching allocator gives: only the
neighbours change), each with a border on both sides that holds a known fill, and checks after the call that

  * every border byte still is its fill (nothing was written outside an output),
  * every ``in`` operand still has the bits that were placed.

A stray READ shows in the result instead, which ``run_three_ways`` compares bit for bit with a plain run: fill 1 (quiet NaN, mask bytes
0xFF = "valid", integers 0x7f..ff) poisons a value that is multiplied by zero or gates something; fill 2 (the largest finite float,
mask bytes 0, integers 0) changes a comparison or a maximum, which a NaN would lose and thereby hide.

A border is at least 64 KiB and at least 256 rows of its operand's own row pitch -- twice the tallest tile any kernel of the library
uses -- so that a plausible overrun lands inside the arena and in nobody else's memory.  That is a safety condition, not a parameter.

What this cannot see: a stray read whose value a select discards leaves no trace in either run, and the library's own scratch is not
under the arena's control.  It bounds which memory can influence a result or be written; it is no proof of memory safety.
"""
import torch

ALIGN = 512
MIN_BORDER = 64 * 1024
BORDER_ROWS = 256
PLAIN_SLACK = 4096            # zeroed bytes on each side of a separately allocated operand of the plain run
ROLES = ('in', 'out', 'inout')
FILLS = (1, 2)

_INT = {torch.int32: torch.int32, torch.int64: torch.int64, torch.float32: torch.int32, torch.uint8: torch.uint8, torch.bool: torch.uint8}
# dtype -> (fill 1, fill 2) as the integer of the same width
_FILL = {
    torch.float32: (0x7fc00000, 0x7f7fffff),
    torch.uint8: (0xFF, 0x00),
    torch.bool: (0xFF, 0x00),
    torch.int32: (0x7fffffff, 0),
    torch.int64: (0x7fffffffffffffff, 0),
}
# what an ``out`` operand holds before the call (the plain run starts from the same bits, so a part the export leaves alone compares equal)
_SENTINEL = {torch.float32: 0x7fc00000, torch.uint8: 0xA5, torch.bool: 0xA5, torch.int32: 0x5A5A5A5A, torch.int64: 0x5A5A5A5A5A5A5A5A}


class ArenaError(AssertionError):
    pass


class BorderError(ArenaError):
    """a byte of a border no longer is its fill: something was stored outside an operand"""


class InputError(ArenaError):
    """an ``in`` operand no longer has the bits that were placed"""


class OutputMismatch(ArenaError):
    """an ``out`` / ``inout`` operand of an arena run differs from the plain run; ``.fill`` says which run"""

    def __init__(self, msg, fill):
        super().__init__(msg)
        self.fill = fill


def _round_up(n, a):
    return (n + a - 1) // a * a


def _bits(t):
    """the tensor's bytes, flat (a bool or float view never meets a comparison of values: NaN == NaN here)"""
    return t.contiguous().reshape(-1).view(torch.uint8)


def _int_fill(region_u8, dtype, value):
    it = _INT[dtype]
    region_u8.view(it).fill_(value if it != torch.uint8 else value & 0xFF)


class Arena:
    def __init__(self, device, fill):
        assert fill in FILLS
        self.device = torch.device(device)
        self.fill = fill
        self._ops = []            # dict(name, cpu, role, pitch, off, nbytes, lo, hi): border bytes [lo, off) and [off + nbytes, hi)
        self._end = 0
        self.buf = None
        self._expect = None
        self._views = {}

    # ---- declaring -----------------------------------------------------------------------------------------------
    def place(self, name, cpu_tensor, role, row_bytes=None):
        """declare an operand; ``row_bytes``: its row pitch if that is not its last dimension (a channel-major (C, T) operand: T * 4)"""
        assert self.buf is None, 'place() after build()'
        assert role in ROLES, role
        assert cpu_tensor.dtype in _FILL, f'{name}: no fill defined for {cpu_tensor.dtype}'
        assert all(o['name'] != name for o in self._ops), name
        t = cpu_tensor.detach().cpu().contiguous()
        pitch = row_bytes or (t.shape[-1] if t.dim() >= 2 else 1) * t.element_size()
        border = _round_up(max(MIN_BORDER, BORDER_ROWS * pitch), ALIGN)
        lo = self._end
        off = lo + border
        nbytes = t.numel() * t.element_size()
        hi = _round_up(off + nbytes + border, ALIGN)
        self._ops.append(dict(name=name, cpu=t, role=role, pitch=pitch, off=off, nbytes=nbytes, lo=lo, hi=hi))
        self._end = hi
        return self

    def build(self):
        """allocate the buffer, write the fills, the sentinels and the operands; returns {name: view}"""
        assert self.buf is None
        host = torch.zeros(self._end, dtype=torch.uint8)
        for o in self._ops:
            t = o['cpu']
            assert o['off'] % ALIGN == 0 and o['lo'] % ALIGN == 0 and o['hi'] % ALIGN == 0
            assert o['off'] - o['lo'] >= max(MIN_BORDER, BORDER_ROWS * o['pitch']) <= o['hi'] - o['off'] - o['nbytes']
            _int_fill(host[o['lo']:o['off']], t.dtype, _FILL[t.dtype][self.fill - 1])
            _int_fill(host[o['off'] + o['nbytes']:o['hi']], t.dtype, _FILL[t.dtype][self.fill - 1])
            body = host[o['off']:o['off'] + o['nbytes']]
            if o['role'] == 'out':
                _int_fill(body, t.dtype, _SENTINEL[t.dtype])
            else:
                body.copy_(_bits(t))
        self.buf = host.to(self.device) if self.device.type != 'cpu' else host
        self._expect = self.buf.clone()
        for o in self._ops:
            t = o['cpu']
            self._views[o['name']] = self.buf[o['off']:o['off'] + o['nbytes']].view(t.dtype).view(t.shape)
        return dict(self._views)

    def __getitem__(self, name):
        return self._views[name]

    def update(self, name, cpu_tensor):
        """rewrite an ``in`` / ``inout`` operand whose content depends on where the arena lies (a table of device addresses)"""
        o = next(o for o in self._ops if o['name'] == name)
        assert o['role'] != 'out' and cpu_tensor.dtype == o['cpu'].dtype and cpu_tensor.shape == o['cpu'].shape
        o['cpu'] = cpu_tensor.detach().cpu().contiguous()
        self._views[name].copy_(o['cpu'])
        self._expect[o['off']:o['off'] + o['nbytes']].copy_(self.buf[o['off']:o['off'] + o['nbytes']])

    # ---- checking -------------------------------------------------------------------------------------------------
    def verify(self):
        """after the call and a device synchronise: borders and ``in`` operands bit-identical to what build() wrote"""
        if self.device.type == 'cuda':
            torch.cuda.synchronize()
        want = self._expect.clone()
        for o in self._ops:
            if o['role'] != 'in':
                want[o['off']:o['off'] + o['nbytes']] = self.buf[o['off']:o['off'] + o['nbytes']]
        if torch.equal(self.buf, want):
            return
        for o in self._ops:                    # say where
            for side, a, b in (('before', o['lo'], o['off']), ('after', o['off'] + o['nbytes'], o['hi'])):
                bad = (self.buf[a:b] != self._expect[a:b]).nonzero()
                if bad.numel():
                    first, last = int(bad[0]), int(bad[-1])
                    at = first - (o['off'] - a) if side == 'before' else first
                    raise BorderError(f"border {side} '{o['name']}' ({o['role']}) changed: {bad.numel()} bytes, the first at byte {at:+d} "
                                      f"relative to the operand's {'start' if side == 'before' else 'end'}, the last {last - first} bytes further "
                                      f"(fill {self.fill}, row pitch {o['pitch']} bytes)")
        for o in self._ops:
            if o['role'] == 'in':
                a, b = o['off'], o['off'] + o['nbytes']
                bad = (self.buf[a:b] != self._expect[a:b]).nonzero()
                if bad.numel():
                    raise InputError(f"input '{o['name']}' was modified: {bad.numel()} bytes, the first at byte {int(bad[0])} (fill {self.fill})")
        raise ArenaError('arena changed outside every declared region')     # (unreachable: the regions tile the buffer)

    def outputs(self):
        return {o['name']: self._views[o['name']] for o in self._ops if o['role'] != 'in'}


def plain_operands(specs, device):
    """the operands of the plain run: every one a separate allocation (its own zeroed buffer, at a 512-byte offset), ``out`` operands
    pre-filled with the sentinel of the arena runs.  specs: [(name, cpu_tensor, role[, row_bytes])]"""
    views, keep = {}, []
    for name, t, role, *_ in specs:
        t = t.detach().cpu().contiguous()
        nbytes = t.numel() * t.element_size()
        host = torch.zeros(2 * PLAIN_SLACK + _round_up(nbytes, ALIGN), dtype=torch.uint8)
        body = host[PLAIN_SLACK:PLAIN_SLACK + nbytes]
        if role == 'out':
            _int_fill(body, t.dtype, _SENTINEL[t.dtype])
        else:
            body.copy_(_bits(t))
        buf = host.to(device)
        keep.append(buf)
        views[name] = buf[PLAIN_SLACK:PLAIN_SLACK + nbytes].view(t.dtype).view(t.shape)
    return views, keep


def _sync(device):
    if torch.device(device).type == 'cuda':
        torch.cuda.synchronize()


def run_three_ways(specs, call, device, fixup=None):
    """(a) a plain run on separately allocated operands, (b) an arena run with fill 1, (c) an arena run with fill 2.

    specs : [(name, cpu_tensor, role[, row_bytes])]
    call  : call(views) -> return code (0 = success); views maps every name to its tensor on ``device``
    fixup : optional fixup(views, update) run before the call, for operands that hold device addresses of other operands;
            update(name, cpu_tensor) rewrites one

    Raises OutputMismatch if an ``out`` / ``inout`` operand of (b) or (c) differs in any bit from (a), BorderError / InputError from
    verify().  Returns the outputs of the plain run (on ``device``)."""
    views, keep = plain_operands(specs, device)
    if fixup is not None:
        fixup(views, lambda name, t: views[name].copy_(t))
    rc = call(views)
    _sync(device)
    assert rc == 0 or rc is None, f'plain run: return code {rc}'
    plain = {name: views[name] for name, _, role, *_ in specs if role != 'in'}
    for fill in FILLS:
        ar = Arena(device, fill)
        for name, t, role, *rest in specs:
            ar.place(name, t, role, *rest)
        v = ar.build()
        if fixup is not None:
            fixup(v, ar.update)
        rc = call(v)
        _sync(device)
        assert rc == 0 or rc is None, f'arena run, fill {fill}: return code {rc}'
        for name, got in ar.outputs().items():
            a, b = _bits(got), _bits(plain[name])
            if not torch.equal(a, b):
                bad = (a != b).nonzero()
                es = got.element_size()
                raise OutputMismatch(f"fill {fill}: '{name}' differs from the plain run in {bad.numel()} bytes, the first in element "
                                     f"{int(bad[0]) // es} of {got.numel()} (shape {tuple(got.shape)})", fill)
        ar.verify()
    return plain
