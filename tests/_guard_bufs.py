"""Guarded device buffers of integer operands, shared by the kernel tests that go through the C ABI (tests/test_neighbor_kernels_gpu.py,
tests/test_ingest_geometry_gpu.py): the data sits between two bands of a sentinel that no kernel writes, so a store or -- for an
input that must come back bit for bit -- a stray write one element outside the operand shows.  `_bounds.Buf` is the same for floats,
`_store_rows.IntBuf` for int64 words.  Helpers only, no test functions; importable without a GPU."""
import torch


class ByteBuf:
    """uint8 `.t` [n] inside guard bands of 0xA5, holding `values`; `shift` moves the data off 16-byte alignment.  An input is held
    to `intact()` (guards and content); a destination is built from its prefill and held to `guards_intact()`."""

    def __init__(self, values, device, guard=65536, shift=0):
        self.n, self.g = values.numel(), guard + shift
        self.raw = torch.full((self.n + 2 * guard + shift,), 0xA5, dtype=torch.uint8, device=device)
        self.t = self.raw[self.g:self.g + self.n]
        self.t.copy_(values.reshape(-1))
        self.want = values.reshape(-1).clone()

    def guards_intact(self):
        return bool((self.raw[:self.g] == 0xA5).all()) and bool((self.raw[self.g + self.n:] == 0xA5).all())

    def intact(self):
        return self.guards_intact() and torch.equal(self.t.cpu(), self.want)


class Int32Buf:
    """int32 `.t` [n] inside guard bands of 0x5A5A5A5A, holding `values` (inputs: the kernels read these tables and never write
    them)."""
    PAT = 0x5A5A5A5A

    def __init__(self, values, device, guard=16384):
        self.n, self.g = values.numel(), guard
        self.raw = torch.full((self.n + 2 * guard,), self.PAT, dtype=torch.int32, device=device)
        self.t = self.raw[guard:guard + self.n]
        self.t.copy_(values.reshape(-1))
        self.want = values.reshape(-1).clone()

    def intact(self):
        return bool((self.raw[:self.g] == self.PAT).all()) and bool((self.raw[self.g + self.n:] == self.PAT).all()) and \
            torch.equal(self.t.cpu(), self.want)
