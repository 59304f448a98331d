"""A stand-in for `torch` inside e4s_amd.kernels that puts every tensor a wrapper allocates (outputs and workspaces) between two bands of
a sentinel value, so that a write next to a tensor and an element left unwritten both show.  A plain helper module of the GPU kernel
tests (tests/test_gpu_gen_backward_kernels.py, tests/test_gpu_encoder_backward_kernels.py, tests/test_gpu_encoder_forward_kernels.py,
tests/test_gpu_criteria_kernels.py); it holds no test."""
import torch

DEV = "cuda"
SENTINEL = 12345.0          # in the bands of a floating-point buffer; its inside starts as NaN
PAD = 64                    # elements on either side of a guarded tensor (keeps the 16-byte alignment of the vector kernels)
INT_SENTINEL = 0x3c3c3c3c   # in the bands of an integer buffer
INT_POISON = -0x5a5a5a5a    # the inside of an integer buffer before the kernel runs: no count and no index has this value
U8_SENTINEL = 0x3c        # in the bands of a uint8 buffer (the max pools' window codes are 0 .. 8)
U8_POISON = 0xa5          # the inside of a uint8 buffer before the kernel runs: no window code has this value
_FLOATS = (torch.float32, torch.float64)
_INTS = (torch.int32,)
_BYTES = (torch.uint8,)


def _fill(dtype):
    """(band value, inside value) of a guarded buffer of `dtype`"""
    if dtype in _FLOATS:
        return SENTINEL, float("nan")
    return (INT_SENTINEL, INT_POISON) if dtype in _INTS else (U8_SENTINEL, U8_POISON)


class _GuardedTorch:
    """Stands in for `torch` inside e4s_amd.kernels: every tensor a wrapper allocates (outputs and workspaces) is the middle of a
    sentinel-filled buffer and starts as NaN (fp32, fp64), INT_POISON (int32) or U8_POISON (uint8), so a write next to it and an element left unwritten
    both show."""

    def __init__(self):
        self.bufs = []

    def __getattr__(self, name):
        return getattr(torch, name)

    def empty(self, *shape, device=None, dtype=torch.float32):
        shape = tuple(shape[0]) if len(shape) == 1 and isinstance(shape[0], (tuple, list, torch.Size)) else tuple(int(v) for v in shape)
        assert dtype in _FLOATS or dtype in _INTS or dtype in _BYTES, dtype
        n = 1
        for v in shape:
            n *= v
        band, inside = _fill(dtype)
        buf = torch.full((n + 2 * PAD,), band, device=device, dtype=dtype)
        buf[PAD:PAD + n] = inside
        self.bufs.append((buf, n))
        return buf[PAD:PAD + n].view(shape)

    def empty_like(self, t):
        return self.empty(*t.shape, device=t.device, dtype=t.dtype)

    def place(self, t):
        """a copy of `t` on the device inside a guarded buffer (for tensors a kernel updates in place)"""
        out = self.empty(*t.shape, device=DEV, dtype=t.dtype)
        out.copy_(t)
        return out

    def insides(self, dtype):
        """the guarded tensors of `dtype` allocated since the last check(), flat, in allocation order"""
        return [buf[PAD:PAD + n] for buf, n in self.bufs if buf.dtype == dtype]

    def check(self):
        torch.cuda.synchronize()
        for buf, n in self.bufs:
            band = _fill(buf.dtype)[0]
            assert bool((buf[:PAD] == band).all()) and bool((buf[PAD + n:] == band).all()), "a neighbour of an output was written"
        self.bufs.clear()


def unwritten(t):
    """number of elements of a guarded tensor that still hold what empty() put there"""
    return int(torch.isnan(t).sum()) if t.dtype in _FLOATS else int((t == _fill(t.dtype)[1]).sum())
