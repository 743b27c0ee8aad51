"""Batch sharding of enhance() across the GPUs of one node.

Every clip is independent end to end (per-clip normalisation, per-sample GroupNorm, shared deterministic time
embedding, convolution algorithm chosen by IMAGE size only), so the only communication is moving waveforms: rank r
processes clips [lo, hi) of the global batch and the results are all-gathered (ONE `all_gather_into_tensor` per call).
No collective sits on the data path of the solver itself.  Works with the `nccl` (= RCCL over xGMI) backend on GPUs and
with `gloo` (CPU tensors, or GPU tensors staged through the host) in the tests.

    out = sharded_enhance(model, y, N=6, solver="euler", seed=1234)     # every rank gets all B waveforms

N-GPU == 1-GPU, bit for bit: the initial noise of clip i (the reference draws it inside enhance from the device RNG,
flowdec/model.py:512,530-536) depends on the GLOBAL clip index i only -- either sliced from a caller-provided global
`noise` tensor, or drawn from the per-clip stream (seed, i) -- never on the rank layout.

The corpus path shards by WORK instead of by count: `sharded_enhance_batch` takes clips of any lengths (T_pad buckets cut into ragged
batches, the batches spread over the ranks by `balance`), `sharded_enhance_long` the (channel, row) jobs of one long recording.  Both
use the library's seeded noise only, and both return what one process returns, bit for bit, for every world size.
"""
import time
from typing import Callable, List, Optional, Sequence, Tuple

import torch

from .batching import plan_clip_batches
from .model import RegressionModel
from .noise import clip_seed


def shard_range(n_items: int, rank: int, world: int) -> Tuple[int, int]:
    """Contiguous, balanced split: the first (n_items % world) ranks get one extra item."""
    base, extra = divmod(n_items, world)
    lo = rank * base + min(rank, extra)
    return lo, lo + base + (1 if rank < extra else 0)


def shard_sizes(n_items: int, world: int) -> List[int]:
    return [shard_range(n_items, r, world)[1] - shard_range(n_items, r, world)[0] for r in range(world)]


def _world(group=None):
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized():
        return dist.get_world_size(group), dist.get_rank(group)
    return 1, 0


def _needs_host_staging(group=None) -> bool:
    """True when the group's collectives cannot take device tensors (gloo).  Composite backend strings such as
    'cpu:gloo,cuda:nccl' carry a device backend: only a plain 'gloo' group has none."""
    import torch.distributed as dist
    b = str(dist.get_backend(group)).lower()
    return "nccl" not in b and "cuda:" not in b


def all_gather_shards(local: torch.Tensor, n_items: int, group=None) -> torch.Tensor:
    """Rank r holds items shard_range(n_items, r, world) of a [n_items, ...] tensor -> the whole tensor on every rank.
    One `all_gather_into_tensor` into a [world, max_shard, ...] buffer; with an even split the result is a view of that
    buffer (no further copy), with an uneven one the padding rows are dropped by one index_select.  Runs the collective
    even at world size 1 when a process group exists (that is how the RCCL path is exercised on a 1-GPU box)."""
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized()):
        raise RuntimeError("all_gather_shards needs an initialised process group (torch.distributed.init_process_group)")
    world, rank = _world(group)
    sizes = shard_sizes(n_items, world)
    assert local.shape[0] == sizes[rank], f"rank {rank}: local shard has {local.shape[0]} items, expected {sizes[rank]}"
    pad, tail = max(sizes), tuple(local.shape[1:])
    if local.shape[0] == pad:
        send = local.contiguous()
    else:
        send = local.new_zeros((pad,) + tail)
        send[: local.shape[0]] = local
    if send.is_cuda and _needs_host_staging(group):   # gloo moves host memory: stage device tensors through the host
        out = send.new_empty((world * pad,) + tail, device="cpu")
        dist.all_gather_into_tensor(out, send.cpu(), group=group)
        out = out.to(send.device)
    else:
        out = local.new_empty((world * pad,) + tail)
        dist.all_gather_into_tensor(out, send, group=group)
    if all(s == pad for s in sizes):
        return out
    keep = torch.cat([torch.arange(r * pad, r * pad + s) for r, s in enumerate(sizes)]).to(out.device)
    return out.index_select(0, keep)


def sharded_apply(fn: Callable[[torch.Tensor], torch.Tensor], y: torch.Tensor, group=None, always_gather: bool = False) -> torch.Tensor:
    """Apply `fn` (e.g. `lambda yb: model.enhance(yb, N=6, noise=...)`) to this rank's slice of the batch dimension of `y`
    and return the full result on every rank.  `fn` must map [b, ...] -> [b, ...] with the same trailing shape.
    Without a process group (or with one rank, unless `always_gather`) this is just `fn(y)`."""
    world, rank = _world(group)
    if world == 1 and not always_gather:
        return fn(y)
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized()):
        raise RuntimeError("sharded_apply(always_gather=True) needs an initialised process group")
    lo, hi = shard_range(y.shape[0], rank, world)
    # (an idle rank -- fewer clips than ranks -- still takes part in the collective; `fn` keeps the trailing shape, dtype and device)
    local = fn(y[lo:hi]) if hi > lo else y.new_zeros((0,) + tuple(y.shape[1:]))
    return all_gather_shards(local, y.shape[0], group)


def clip_noise(seed: int, index: int, shape, device) -> torch.Tensor:
    """The initial noise of GLOBAL clip `index`: complex64 standard normal of `shape` from its own Philox stream
    (seed, index) -- the same values whatever the batch, the shard or the rank the clip is processed in."""
    g = torch.Generator(device=device)
    g.manual_seed((int(seed) * 1000003 + int(index)) & 0x7FFFFFFFFFFFFFFF)
    return torch.randn(shape, dtype=torch.complex64, device=device, generator=g)


def sharded_enhance(model, y: torch.Tensor, N: int = 50, solver: str = "euler", noise: Optional[torch.Tensor] = None,
                    seed: Optional[int] = None, generator: Optional[torch.Generator] = None, group=None, always_gather: bool = False,
                    stats: Optional[dict] = None, rng: str = "torch", step_control: Optional[str] = None, **enhance_kwargs) -> torch.Tensor:
    """`model.enhance(y, N=N, solver=solver)` for a global batch y [B, 1, L] sharded by clip over the ranks of `group`;
    every rank returns all B enhanced waveforms [B, 1, L] on y's device.  Result == the single-process call, bit for bit:

      noise=      global initial noise [B, 1, F, T_pad] complex64 (every rank passes the same tensor or at least its own
                  rows): rank r uses rows [lo, hi);
      seed=       clip i draws from the stream (seed, i) (`clip_noise`); the default when nothing is given: rank 0 draws a
                  seed and broadcasts it.  With rng="native" the noise is the library's own instead (`model.enhance(seed=)`):
                  global clip i uses `flowdec_amd.noise.clip_seed(seed, i)` and no noise tensor is drawn or copied;
      generator=  one generator seeded IDENTICALLY on every rank: the full [B, ...] noise is drawn and sliced, which equals
                  `model.enhance(y, generator=g)` of a single process (costs B x 1.5 MB per second of audio of device memory).

    The adaptive solvers ('dopri5', 'tsit5') keep that promise with step_control='clip' only (every clip under its own step controller,
    `FlowModel.enhance`): the default controller takes one error ratio over a rank's whole shard, so its result depends on the sharding.
    `step_control` is forwarded on every noise path.

    y may live on the host (pinned or not): only this rank's rows are copied to the model's device, and the gathered result
    is copied back -- the "H2D of waveform -> D2H of waveform" path of SURVEY 8(d).  `stats`, if given, receives
    {"local_s", "gather_s"} host-clock seconds (it synchronises the device, use it for measurements only)."""
    if y.ndim != 3 or y.shape[1] != 1:
        raise RuntimeError(f"sharded_enhance expects a batch [B, 1, L] (got {tuple(y.shape)})")
    if rng not in ("torch", "native"):
        raise ValueError(f"rng must be 'torch' or 'native' (got {rng!r})")
    if rng == "native" and (noise is not None or generator is not None):
        raise ValueError("rng='native' draws from seed=: it takes neither noise= nor generator=")
    if step_control is not None:
        enhance_kwargs = dict(enhance_kwargs, step_control=step_control)
    world, rank = _world(group)
    B, Lw = y.shape[0], y.shape[-1]
    lo, hi = shard_range(B, rank, world)
    dev = model.device
    out_device = y.device
    t0 = time.perf_counter() if stats is not None else 0.0
    local = None
    if rng == "native":
        if seed is None:
            seed = _shared_seed(dev, group)   # (every rank, idle ones included, takes part in the broadcast)
        if hi > lo:
            local = model.enhance(y[lo:hi].to(dev, non_blocking=True), N=N, solver=solver, seed=[clip_seed(seed, i) for i in range(lo, hi)],
                                  **enhance_kwargs)
    elif hi > lo:
        yl = y[lo:hi].to(dev, non_blocking=True)
        if noise is not None:
            nz = noise[lo:hi]
        else:
            cfg = model.feature_extractor._cfg()
            n_freq, T = cfg["n_fft"] // 2 + 1, 1 + Lw // cfg["hop"]      # fd_num_frames / fd_padded_frames (pad_spec: multiple of 64)
            Tp = 64 * ((T + 63) // 64)
            if generator is not None:
                nz = _full_draw(generator, B, n_freq, Tp, dev)[lo:hi]
            else:
                if seed is None:
                    seed = _shared_seed(dev, group)
                nz = torch.stack([clip_noise(seed, i, (1, n_freq, Tp), dev) for i in range(lo, hi)])
        local = model.enhance(yl, N=N, solver=solver, noise=nz, **enhance_kwargs)
    elif noise is None and generator is not None:
        # idle rank (fewer clips than ranks): draw and discard the full noise, so that the generators of all ranks stay identical for
        # the next call -- the contract of `generator=`
        cfg = model.feature_extractor._cfg()
        T = 1 + Lw // cfg["hop"]
        _full_draw(generator, B, cfg["n_fft"] // 2 + 1, 64 * ((T + 63) // 64), dev)
    elif noise is None and seed is None:
        _shared_seed(dev, group)   # idle rank: still takes part in the seed broadcast
    if stats is not None:
        if dev.type == "cuda":
            torch.cuda.synchronize(dev)
        t1 = time.perf_counter()
        stats["local_s"] = stats.get("local_s", 0.0) + (t1 - t0)
    if world == 1 and not always_gather:
        out = local
    else:
        import torch.distributed as dist
        if not (dist.is_available() and dist.is_initialized()):
            raise RuntimeError("sharded_enhance(always_gather=True) needs an initialised process group")
        if local is None:
            local = torch.empty((0, 1, Lw), dtype=torch.float32, device=dev)
        out = all_gather_shards(local, B, group)
    if out.device != out_device:
        out = out.to(out_device)
    if stats is not None:
        if dev.type == "cuda":
            torch.cuda.synchronize(dev)
        stats["gather_s"] = stats.get("gather_s", 0.0) + (time.perf_counter() - t1)
    return out


def _full_draw(generator: torch.Generator, B: int, n_freq: int, Tp: int, dev) -> torch.Tensor:
    """The [B, 1, F, T_pad] complex64 noise of the whole global batch from `generator` (on the generator's device)."""
    return torch.randn((B, 1, n_freq, Tp), dtype=torch.complex64, device=generator.device, generator=generator).to(dev)


def _shared_seed(dev, group=None) -> int:
    """A fresh seed that every rank agrees on (rank 0 draws, one 8-byte broadcast)."""
    import torch.distributed as dist
    world, rank = _world(group)
    s = torch.randint(0, 2 ** 62, (1,), dtype=torch.int64)
    if world > 1:
        s = s if _needs_host_staging(group) else s.to(dev)
        dist.broadcast(s, src=dist.get_global_rank(group, 0) if group is not None else 0, group=group)
    return int(s.item())


# ------------------------------------------------------------------------------------------------
# the corpus path: clips of any lengths, one long recording
# ------------------------------------------------------------------------------------------------
def balance(costs: Sequence[float], world: int) -> List[List[int]]:
    """Assigns items to ranks: longest cost first, each to the rank with the least load so far.  Equal costs go in item order (lower
    index first), equal loads to the lower rank; every rank's list comes back in ascending item order.  A pure function of its
    arguments: every rank computes the same plan from the same costs, nothing is communicated.

    Guarantees: every item appears exactly once; world == 1 gives [list(range(n))]; ranks may be empty (fewer items than ranks, or zero
    costs elsewhere); max load <= sum(costs) / world + max(costs), the list-scheduling bound (the rank that ends up fullest was the
    least loaded one, so at most the mean, when it took its last item)."""
    world = int(world)
    if world < 1:
        raise ValueError(f"balance: world must be >= 1 (got {world})")
    if any(c < 0 for c in costs):
        raise ValueError("balance: costs must be >= 0")
    load, plan = [0] * world, [[] for _ in range(world)]
    for i in sorted(range(len(costs)), key=lambda i: (-costs[i], i)):
        r = min(range(world), key=lambda r: (load[r], r))
        load[r] += costs[i]
        plan[r].append(i)
    return [sorted(p) for p in plan]


def sharded_enhance_batch(model, clips, group=None, batch_clips: int = 8, seed: Optional[int] = None, seeds=None, always_gather: bool = False,
                          stats: Optional[dict] = None, **enhance_kwargs) -> List[torch.Tensor]:
    """`[model.enhance(c, seed=[s_i], ...) for c in clips]` for a list of clips of ANY lengths ([L], [1, L] or [1, 1, L]), sharded over
    the ranks of `group`; every rank passes the same list (host tensors are fine) and returns all clips, each with the shape and on the
    device of its input.  `model` is a FlowModel, a ScoreModel or a RegressionModel (anything with their `enhance_batch`).

    The clips are bucketed by T_pad and cut into ragged batches of at most `batch_clips` (`plan_clip_batches`); a batch costs
    clips x T_pad, `balance` spreads the batches, and each rank runs its own through `model.enhance_batch` -- where every clip gets the
    arithmetic of its own one-clip call.  ONE `all_gather_into_tensor` then moves the waveforms, padded to the longest clip (gloo: staged
    through the host); the result is copied out of the gathered buffer, so it is the one-clip result bit for bit, the sign of a zero
    included, for every world size.

    Noise is the library's own: `seeds` = one 64-bit seed per clip, or `seed` = an int (clip i uses `noise.clip_seed(seed, i)`); with
    neither, rank 0 draws a seed and broadcasts it (idle ranks take part).  A RegressionModel draws no noise and takes none of them.
    `noise=` / `generator=` are refused: a shared generator's stream depends on the order in which the clips are processed, which is
    what sharding changes.  The adaptive solvers need step_control='clip' (`enhance_batch` enforces it).

    Without a process group (world 1) the clips still run bucketed and batched; there is no collective unless `always_gather`.
    `stats`, if given, receives {"local_s", "gather_s"} like `sharded_enhance`, plus "plan" (every batch as a list of clip indices) and
    "mine" (the positions in the plan of the batches this rank ran)."""
    for k in ("noise", "generator"):
        if enhance_kwargs.get(k) is not None:
            raise ValueError(f"sharded_enhance_batch takes seed= / seeds= only, not {k}=: a generator's stream (and a noise list drawn from one) "
                             f"depends on the order the clips are processed in, which the sharding changes; the library's seeded noise "
                             f"belongs to the clip")
        enhance_kwargs.pop(k, None)
    clips = list(clips)
    n = len(clips)
    world, rank = _world(group)
    dev = model.device
    draws_noise = not isinstance(model, RegressionModel)
    if not draws_noise:
        seeds = None
    elif seeds is not None:
        if seed is not None:
            raise ValueError("sharded_enhance_batch: pass seed= or seeds=, not both")
        seeds = [int(s) for s in (seeds.view(torch.int64).tolist() if isinstance(seeds, torch.Tensor) else seeds)]   # (two's complement)
        if len(seeds) != n:
            raise ValueError(f"sharded_enhance_batch: {len(seeds)} seeds for {n} clips")
    else:
        if seed is None:
            seed = _shared_seed(dev, group)   # (every rank, idle ones included, takes part in the broadcast)
        seeds = [clip_seed(seed, i) for i in range(n)]
    lens = [int(c.numel()) for c in clips]
    batches = plan_clip_batches(lens, model.feature_extractor._cfg()["hop"], batch_clips)
    plan, costs = [idx for _, idx in batches], [len(idx) * tp for tp, idx in batches]
    owner = balance(costs, world)
    t0 = time.perf_counter() if stats is not None else 0.0
    local = {}
    for b in owner[rank]:
        idx = plan[b]
        kw = dict(enhance_kwargs, seeds=[seeds[i] for i in idx]) if draws_noise else enhance_kwargs
        outs = model.enhance_batch([clips[i].to(dev, non_blocking=True) for i in idx], **kw)
        local.update(zip(idx, outs))
    if stats is not None:
        if dev.type == "cuda":
            torch.cuda.synchronize(dev)
        t1 = time.perf_counter()
        stats["local_s"] = stats.get("local_s", 0.0) + (t1 - t0)
        stats["plan"], stats["mine"] = plan, list(owner[rank])
    if world == 1 and not always_gather:
        res = [local[i].reshape(clips[i].shape).to(clips[i].device) for i in range(n)]
    else:
        import torch.distributed as dist
        if not (dist.is_available() and dist.is_initialized()):
            raise RuntimeError("sharded_enhance_batch(always_gather=True) needs an initialised process group")
        # rank r's clips, in the order of its batches, are the slots of row r of a [world, slots, longest clip] buffer
        slots = [[i for b in owner[r] for i in plan[b]] for r in range(world)]
        n_slots, l_max = max(max(len(s) for s in slots), 1), max(lens + [1])
        send = torch.zeros(n_slots, l_max, dtype=torch.float32, device=dev)
        for k, i in enumerate(slots[rank]):
            send[k, :lens[i]].copy_(local[i].reshape(-1))
        if send.is_cuda and _needs_host_staging(group):   # gloo moves host memory: stage device tensors through the host
            out = torch.empty(world * n_slots, l_max, dtype=torch.float32)
            dist.all_gather_into_tensor(out, send.cpu(), group=group)
        else:
            out = send.new_empty(world * n_slots, l_max)
            dist.all_gather_into_tensor(out, send, group=group)
        res = [None] * n
        for r in range(world):
            for k, i in enumerate(slots[r]):
                res[i] = out[r * n_slots + k, :lens[i]].clone().reshape(clips[i].shape).to(clips[i].device)
    if stats is not None:
        if dev.type == "cuda":
            torch.cuda.synchronize(dev)
        stats["gather_s"] = stats.get("gather_s", 0.0) + (time.perf_counter() - t1)
    return res


def sharded_enhance_long(model, y: torch.Tensor, seed=None, group=None, always_gather: bool = False, row_frames: int = 3712,
                         halo_frames: int = 256, xfade: Optional[int] = None, **enhance_long_kwargs) -> torch.Tensor:
    """`model.enhance_long(y, seed=seed, ...)` with the (channel, row) jobs of the ONE recording y ([L], [1, L] or [C, 1, L]) sharded over
    the ranks of `group`: rank r runs the contiguous jobs `shard_range(jobs, r, world)` (`FlowModel.enhance_long_rows`), the row
    outputs are all-gathered (`all_gather_shards`, one collective) and every rank stitches the recording (`enhance_long_stitch`).  A row
    depends on (recording, seed, absolute frame) only, and every rank takes the recording's normalisation from the whole recording (a
    maximum: order-free, the same bits everywhere), so the result equals the one-process call bit for bit for every world size.
    Every rank passes the same y.  seed=None: rank 0 draws one and broadcasts it."""
    world, rank = _world(group)
    if seed is None:
        seed = _shared_seed(model.device, group)
    geometry = dict(row_frames=row_frames, halo_frames=halo_frames, xfade=xfade)
    if world == 1 and not always_gather:
        return model.enhance_long(y, seed=seed, **geometry, **enhance_long_kwargs)
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized()):
        raise RuntimeError("sharded_enhance_long(always_gather=True) needs an initialised process group")
    n_jobs = model.enhance_long_jobs(y, **geometry)
    local = model.enhance_long_rows(y, jobs=shard_range(n_jobs, rank, world), seed=seed, **geometry, **enhance_long_kwargs)
    return model.enhance_long_stitch(y, all_gather_shards(local, n_jobs, group), **geometry)
