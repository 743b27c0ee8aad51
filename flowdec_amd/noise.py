"""Per-clip seeds for the library's own sampler noise (include/flowdec_hip.h, "Seeded noise").

The noise of a clip is a pure function of (clip seed, draw index, frequency row, frame), evaluated on the GPU by the kernel that
consumes it: the same numbers whatever the batch, the T_pad bucket, the shard or the rank the clip is processed in.  This module
holds the host side: `clip_seed` (one run seed -> one 64-bit seed per clip), the conversion of the `seed=` arguments into the
device array the C ABI takes, and `noise_fill` (the same noise written to a buffer, for the entry points that read one).
"""
import torch

from . import _lib as L

_M64 = (1 << 64) - 1
NOISE_GAUSSIAN, NOISE_BITS = 0, 1   # FD_NOISE_*


def _mix64(x: int) -> int:
    """The SplitMix64 output function: a bijection of the 64-bit integers."""
    x = (x + 0x9E3779B97F4A7C15) & _M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & _M64
    return x ^ (x >> 31)


def clip_seed(seed: int, index: int) -> int:
    """The 64-bit seed of clip `index` of a run seeded `seed`: mix(mix(seed) + index).  The run seed is scattered over the 64-bit
    range before the index is added, so neighbouring run seeds do not share clip seeds ((S, i + 1) and (S + 1, i) differ), and the
    outer mix is a bijection, so the clips of one run never collide."""
    return _mix64((_mix64(int(seed) & _M64) + int(index)) & _M64)


def seeds_to_tensor(seed, B: int, device) -> torch.Tensor:
    """`seed=` of the enhance calls -> int64 [B] on `device` holding the clips' 64-bit seeds (two's complement): an int means clip b
    uses clip_seed(seed, b); a sequence of B ints or a uint64 / int64 tensor [B] gives every clip's seed directly."""
    if isinstance(seed, torch.Tensor):
        if seed.dtype not in (torch.int64, torch.uint64) or tuple(seed.shape) != (B,):
            raise RuntimeError(f"seed tensor must be int64 / uint64 of shape [{B}] (got {seed.dtype}, {tuple(seed.shape)})")
        return seed.view(torch.int64).to(device)
    if isinstance(seed, (list, tuple)):
        if len(seed) != B:
            raise RuntimeError(f"one seed per clip: got {len(seed)} seeds for {B} clips")
        vals = [int(s) & _M64 for s in seed]
    else:
        vals = [clip_seed(int(seed), b) for b in range(B)]
    return torch.tensor([v - (1 << 64) if v >> 63 else v for v in vals], dtype=torch.int64).to(device)


def noise_fill(seeds: torch.Tensor, F: int, T_pad: int, draw0: int = 0, n_draws: int = 1, bits: bool = False) -> torch.Tensor:
    """fd_noise_fill: the planes draw0 .. draw0 + n_draws - 1 of the clips seeded `seeds` (int64 [B] on the GPU, see seeds_to_tensor)
    -> complex64 [n_draws, B, 1, F, T_pad], the layout fd_score_enhance consumes ([0] is fd_enhance's); bits=True -> the generator's
    raw words (ra, rb) as int64 [n_draws, B, 1, F, T_pad, 2] (each in [0, 2^32))."""
    L.require_cuda(seeds)
    lib = L.load()
    B = seeds.numel()
    with torch.cuda.device(seeds.device):
        if bits:
            raw = torch.empty(n_draws, B, 1, F, T_pad, 2, dtype=torch.int32, device=seeds.device)
            L.check(lib.fd_noise_fill(L.ptr(raw), L.ptr(seeds), B, F, T_pad, int(draw0), int(n_draws), NOISE_BITS, L.stream()))
            return raw.to(torch.int64) & 0xFFFFFFFF
        out = torch.empty(n_draws, B, 1, F, T_pad, dtype=torch.complex64, device=seeds.device)
        L.check(lib.fd_noise_fill(L.ptr(torch.view_as_real(out)), L.ptr(seeds), B, F, T_pad, int(draw0), int(n_draws), NOISE_GAUSSIAN, L.stream()))
    return out


def exclusive(**given):
    """`seed=`, `noise=` and `generator=` name three different sources of the same noise: at most one may be given."""
    named = [k for k, v in given.items() if v is not None]
    if len(named) > 1:
        raise ValueError("the noise source is ambiguous: pass only one of " + ", ".join(f"{k}=" for k in named))
