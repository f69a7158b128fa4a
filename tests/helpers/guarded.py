"""Run the point-cloud entry points on buffers of exactly the size include/deflow_amd.h states, surrounded by a byte pattern.

The wrappers allocate outputs and workspaces with torch.empty; the caching allocator rounds that up to 512 bytes and hands out
neighbouring blocks of one segment, so a write a few bytes past an output, a workspace carve that is one alignment step short or a tile
loop that reads past an input corrupts (or reads) live memory with every other test green.  ``Guard`` stands between a wrapper and
``_lib.call``:

  ptr    records pointer -> tensor.
  call   for an entry of tests/helpers/abi_sizes.py: asserts that the tensor the wrapper passed spans at least the header's size (a short
         wrapper allocation), copies EVERY sized buffer -- inputs too -- into a region of exactly that size inside one uint8 arena filled
         with a byte pattern, calls the real entry with the region pointers on the same stream, copies outputs, in/out buffers and
         workspaces back (stage chains such as df_dbscan_core / link / finish keep state in the workspace), and asserts that every arena byte
         outside the regions still holds the pattern.  A failure names the entry, the parameter, and the offset and length of the damage.
         Any other entry goes straight through.

The arena's layout is a set of conditions, not measurements: regions are 16-byte aligned at addresses that are 16 mod 32 (nothing gets
more alignment than the header grants), every region has at least PAD = 4096 pattern bytes before and after it, and at least TAIL = 1 MiB
of pattern lies behind the last one, so that a stray write of any plausible size stays inside this one allocation.  An over-read does not
damage anything; it shows as a result that depends on the fill, which is why the tests run every scenario with two fills (0xA5: tiny
negative floats, negative ints; 0x7F: floats of about 3.4e38, large positive ints) and compare the results bit for bit.

It refuses to run while the stream is capturing: it synchronises to read the guard bytes."""
from __future__ import annotations

import sys
from typing import Callable, Dict, List, Optional, Tuple

import torch

import abi_sizes

PAD = 4096
TAIL = 1 << 20


class GuardError(AssertionError):
    pass


def extent(t: torch.Tensor) -> int:
    """bytes the tensor spans from its data pointer (its own strided span, not its storage's)"""
    if t.numel() == 0:
        return 0
    return (sum((n - 1) * s for n, s in zip(t.shape, t.stride())) + 1) * t.element_size()


def raw_bytes(t: torch.Tensor, n: int) -> torch.Tensor:
    """the n bytes from the tensor's data pointer, as a uint8 view of its storage"""
    st = t.untyped_storage()
    flat = torch.empty(0, dtype=torch.uint8, device=t.device).set_(st)
    off = t.data_ptr() - st.data_ptr()
    assert off >= 0 and off + n <= flat.numel(), (off, n, flat.numel())
    return flat[off:off + n]


def same_bits(a: torch.Tensor, b: torch.Tensor) -> bool:
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.numel() == 0:
        return True
    return bool(torch.equal(a.contiguous().reshape(-1).view(torch.uint8), b.contiguous().reshape(-1).view(torch.uint8)))


class Guard:
    def __init__(self, fill: int, real_call: Callable, table: Optional[Dict[str, abi_sizes.Entry]] = None,
                 query: Callable[..., int] = abi_sizes.ws_query):
        assert 0 <= fill <= 255
        self.fill, self.real_call, self.query = fill, real_call, query
        self.table = abi_sizes.TABLE if table is None else table
        self.recorded: Dict[int, torch.Tensor] = {}
        self.seen: List[str] = []                       # the guarded calls, in order
        self.layout: List[Tuple[str, int, int]] = []    # of the last guarded call: (parameter, address, bytes)
        self.arena_span: Tuple[int, int] = (0, 0)       # of the last guarded call: (address, bytes)

    # ---- the two names the op modules import from _lib ----------------------------------------------------------------------------------
    def ptr(self, t: Optional[torch.Tensor]) -> Optional[int]:
        if t is None:
            return None
        self.recorded[t.data_ptr()] = t
        return t.data_ptr()

    def call(self, name: str, *args):
        if name not in self.table:
            return self.real_call(name, *args)
        try:
            return self._guarded(name, args)
        finally:
            self.recorded.clear()

    # ---- one guarded call ---------------------------------------------------------------------------------------------------------------
    def _guarded(self, name: str, args):
        entry = self.table[name]
        if len(args) != len(entry.params) + 1:
            raise GuardError(f"{name}: {len(args)} arguments, the table has {len(entry.params)} and the stream")
        scalars = abi_sizes.scalars_of(entry, args)
        bufs = []                                       # (position, parameter, Buf, tensor, bytes)
        for pos, pname in enumerate(entry.params):
            b = entry.bufs.get(pname)
            if b is None:
                continue
            p = args[pos]
            if p is None or p == 0:
                if not b.nullable:
                    raise GuardError(f"{name}: {pname}: NULL, and the header does not allow that")
                continue
            t = self.recorded.get(p)
            if t is None:
                raise GuardError(f"{name}: {pname}: the pointer {p:#x} was not made by ptr(): the wrapper passed a raw address")
            size = abi_sizes.eval_buf(b, scalars, self.query)
            if size is None:
                if b.role != abi_sizes.IN:
                    raise GuardError(f"{name}: {pname}: only an input may take its extent from the recorded tensor")
                size = extent(t)
            if size < 0:
                raise GuardError(f"{name}: {pname}: the header's size is {size} bytes at {scalars}")
            if extent(t) < size:
                raise GuardError(f"{name}: {pname}: the wrapper passed a tensor of {extent(t)} bytes, the header states {size} "
                                 f"(shape {tuple(t.shape)}, {t.dtype}) at {scalars}")
            bufs.append((pos, pname, b, t, size))
        dev = bufs[0][3].device if bufs else torch.device("cpu")
        if dev.type == "cuda":
            if torch.cuda.is_current_stream_capturing():
                raise GuardError(f"{name}: the guarded call synchronises and cannot run while the stream is capturing")
            if args[-1] != torch.cuda.current_stream(dev).cuda_stream:
                raise GuardError(f"{name}: the wrapper launches on a stream that is not torch's current one")
        for k, (_, na, ba, ta, sa) in enumerate(bufs):  # a written buffer that overlaps another one cannot be carved apart
            for _, nb, bb, tb, sb in bufs[k + 1:]:
                if (ba.role != abi_sizes.IN or bb.role != abi_sizes.IN) and ta.data_ptr() < tb.data_ptr() + sb and \
                        tb.data_ptr() < ta.data_ptr() + sa:
                    raise GuardError(f"{name}: {na} and {nb} overlap and one of them is written")

        total = PAD + sum(s + PAD + 32 for *_, s in bufs) + TAIL
        arena = torch.full((total,), self.fill, dtype=torch.uint8, device=dev)
        base = arena.data_ptr()
        regions = []                                    # (offset, bytes, parameter, Buf, tensor)
        cur = PAD
        for _, pname, b, t, size in bufs:
            cur += (16 - (base + cur)) % 32             # 16-byte aligned, and no more than that
            regions.append((cur, size, pname, b, t))
            cur += size + PAD
        assert total - (regions[-1][0] + regions[-1][1] if regions else 0) >= TAIL
        self.layout = [(pname, base + off, size) for off, size, pname, _, _ in regions]
        self.arena_span = (base, total)

        new = list(args)
        for (pos, *_), (off, size, _, _, t) in zip(bufs, regions):
            if size:
                arena[off:off + size].copy_(raw_bytes(t, size))
            new[pos] = base + off
        rc = self.real_call(name, *new)
        for off, size, _, b, t in regions:
            if size and b.role != abi_sizes.IN:
                raw_bytes(t, size).copy_(arena[off:off + size])
        for off, size, *_ in regions:
            arena[off:off + size].fill_(self.fill)
        bad = arena != self.fill
        if bool(bad.any()):
            raise GuardError(f"{name}: " + self._describe(bad.nonzero().reshape(-1).tolist(), regions))
        self.seen.append(name)
        return rc

    @staticmethod
    def _describe(damaged: List[int], regions) -> str:
        """the first run of damaged bytes, attributed to the region it lies nearest to"""
        first = damaged[0]
        n = 1
        while n < len(damaged) and damaged[n] - damaged[n - 1] <= 16:      # one stray store: a run with small holes
            n += 1
        last = damaged[n - 1]
        best = None
        for off, size, pname, b, _ in regions:
            if first >= off + size:
                d, where = first - (off + size), f"{first - (off + size)} bytes past its end"
            else:
                d, where = off - last, f"{off - first} bytes before its start"
            if best is None or d < best[0]:
                best = (d, f"{pname} ({b.role}, {size} bytes): {last - first + 1} damaged bytes starting {where}")
        more = "" if n == len(damaged) else f"; {len(damaged) - n} more damaged bytes further on"
        return best[1] + more


def install(monkeypatch, fill: int) -> Guard:
    """put a Guard's ``call`` and ``ptr`` in place of the names every op module imported from deflow_amd._lib"""
    import importlib
    from deflow_amd import _lib
    for m in ("args", "augment", "chamfer", "cluster", "decoder", "fastnsf", "floxels", "ground", "mbnsf", "metrics_device", "nsfp", "odometry",
              "pairflow", "pairopt", "refine", "render", "rigid", "submit", "sweeps", "voidmap"):
        importlib.import_module("deflow_amd." + m)
    g = Guard(fill, _lib.call)
    hit = 0
    for mname, mod in list(sys.modules.items()):
        if mod is None or not mname.startswith("deflow_amd.") or mod is _lib:
            continue
        if getattr(mod, "call", None) is _lib.call and getattr(mod, "ptr", None) is _lib.ptr:
            monkeypatch.setattr(mod, "call", g.call)
            monkeypatch.setattr(mod, "ptr", g.ptr)
            hit += 1
    assert hit >= 20, hit
    return g
