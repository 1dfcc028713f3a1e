"""Diagnostic (not a test): one training step of the memory path at the bench shape - forward under autograd +
backward, 64 frames, M=64, D=1024, bf16 - wall time and per-kernel-kind breakdown (HIP events).
usage: python tools/bench_train.py [steps]
env: MEM_TOKENS, HIDDEN, BWD_FUSED; BATCH=B (default 1: the single-video path, the output below) or a list "1,2,4,8": the
row-batched training step (BatchedProjector.step_train) of B distinct videos against the single-video step, the configurations
interleaved round by round in this one process; ms per step and per video, then the kernel table of each.
CHUNKS=3,2,2,1: videos of that many 32-frame chunks each, timed three ways, interleaved round by round in this one process: as ONE
ragged row batch (step_train(ragged=True) on the smallest engine of 2 / 4 / 8 that holds them), under the equal-length grouping
(plan_row_batches over the chunk counts: row batches of equal length plus single videos) and as single videos; ms per pass and per
(video, chunk) step, then the kernel table - launches per pass - of each.
CLIPS=31,27,23,19,16,12,9,5: clips of that many frames each (one chunk of all its frames), timed three ways, interleaved round by
round in this one process after warming up all three: as clip row batches (plan_clip_batches; a group takes ONE
step_train_frames - the variable-length attention forward and backward -, what is left runs under the equal-length grouping),
under the equal-length grouping alone (plan_row_batches over the frame counts: the switch off) and as single videos; ms per pass
and per video, then the kernel table - launches per pass - of each (ROUNDS, default 5 here).  HIDDEN=3584 (heads of 448): the clip
leg runs with ops.set_attention_hd_varlen_train(True) (the variable-length 448 forward and backward), the other two with it off."""
import ctypes, sys, os, time
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import memory_augmented_vlm_amd
from memory_augmented_vlm_amd import _capi as capi
from memory_augmented_vlm_amd.model.memory_module.MemoryController import Config, TransformerProjector

steps = int(sys.argv[1]) if len(sys.argv) > 1 else 3
capi.lib().mavlm_set_attention_bwd_fused(int(os.environ.get("BWD_FUSED", "0")))
M = int(os.environ.get("MEM_TOKENS", "64"))
HID = int(os.environ.get("HIDDEN", "1024"))
c = Config(); c.mm_hidden_size = HID; c.mm_intermediate_size = 4 * HID; c.mm_num_attention_heads = 8
c.num_memory_tokens = M; c.patch_size = 196; c.depth = 2; c.mm_dtype = torch.float32
torch.manual_seed(0)
rm = TransformerProjector(c).cuda().to(torch.bfloat16).train()
x = (torch.randn(64, 196, HID, device="cuda") * 0.5).bfloat16()

def step():
    rm.zero_grad(set_to_none=True)
    rm.memory_cache = []
    for i in range(2):
        cache, _ = rm(x[32 * i:32 * i + 32])
    loss = sum(cm.float().square().mean() for cm in cache)
    loss.backward()
    return loss

def fwd_only():
    with torch.no_grad():
        rm.memory_cache = []
        for i in range(2):
            rm(x[32 * i:32 * i + 32])

BATCHES = [int(b) for b in os.environ.get("BATCH", "1").split(",")]

def kernel_table(fn):
    lib = capi.lib(); nk = len(capi.KERNEL_KINDS)
    ms = (ctypes.c_double * nk)(); ln = (ctypes.c_int64 * nk)(); fl = (ctypes.c_double * nk)(); by = (ctypes.c_double * nk)()
    lib.mavlm_prof_enable(1)
    for _ in range(steps): fn()
    torch.cuda.synchronize()
    capi.check(lib.mavlm_prof_read(ms, ln, fl, by, nk), "prof"); lib.mavlm_prof_enable(0)
    tot = sum(ms)
    for i, name in enumerate(capi.KERNEL_KINDS):
        if ln[i]:
            print(f"{name:18s} launches/step {ln[i]/steps:6.1f}  ms/step {ms[i]/steps:8.3f}  ({100*ms[i]/tot:4.1f}%)  avg {ms[i]/ln[i]*1e3:8.1f} us"
                  + (f"  {fl[i]/(ms[i]*1e-3)/1e12:7.1f} TF" if fl[i] else f"  {by[i]/(ms[i]*1e-3)/1e9:7.1f} GB/s"))
    print(f"sum of HIP kernels {tot/steps:.2f} ms/step (torch glue kernels not included)")
    return tot / steps

if os.environ.get("CLIPS"):
    from memory_augmented_vlm_amd.model import llava_arch as arch
    from memory_augmented_vlm_amd.model.memory_module.MemoryController import BatchedProjector
    frames = [int(v) for v in os.environ["CLIPS"].split(",")]
    vids = [(torch.randn(f, 196, HID, device="cuda") * 0.5).bfloat16() for f in frames]        # distinct clips
    loss_of = lambda mems: sum(cm.float().square().mean() for cm in mems)
    def single_video(v):
        rm.memory_cache = []
        cache, _ = rm(v)
        return loss_of(cache)
    def singles():
        rm.zero_grad(set_to_none=True)
        sum(single_video(v) for v in vids).backward()
    bps = {}
    def engine(size):
        if size not in bps:
            bps[size] = BatchedProjector(rm, size)
        return bps[size]
    def equal_groups(idx):
        """the switch-off grouping of the clips `idx`: row batches of equal frame counts, the rest single videos"""
        batches, alone = arch.plan_row_batches([frames[i] for i in idx])
        loss = 0.0
        for g in batches:
            bp = engine(len(g))
            bp.reset()
            bp.step_train([vids[idx[j]] for j in g])
            loss = loss + sum(loss_of(bp.memory_cache(b)) for b in range(len(g)))
        for j in alone:
            loss = loss + single_video(vids[idx[j]])
        return loss
    def grouped():
        rm.zero_grad(set_to_none=True)
        equal_groups(list(range(len(frames)))).backward()
    cgroups, rest = arch.plan_clip_batches(frames)
    from memory_augmented_vlm_amd import _ops as ops
    wide = HID // 8 == 448           # heads of 448: the clip leg needs ops.set_attention_hd_varlen_train (off by default, and in the other legs)
    def clips():
        rm.zero_grad(set_to_none=True)
        loss = 0.0
        ops.set_attention_hd_varlen_train(wide)
        try:
            for size, g in cgroups:
                bp = engine(size)
                bp.reset()
                bp.step_train_frames([vids[i] for i in g])
                loss = loss + sum(loss_of(bp.memory_cache(b)) for b in range(len(g)))
            if rest:
                loss = loss + equal_groups(rest)
            loss.backward()
        finally:
            ops.set_attention_hd_varlen_train(False)
    fns = {"clips": clips, "grouped": grouped, "singles": singles}
    eq_b, eq_a = arch.plan_row_batches(frames)
    print(f"CLIPS={frames}  M={M} hidden={HID}; clip row batches {[[frames[i] for i in g] for _, g in cgroups]} on engines of "
          f"{[sz for sz, _ in cgroups]}, the rest {[frames[i] for i in rest]}; equal-length grouping (the switch off): row batches "
          f"{[[frames[j] for j in g] for g in eq_b]}, single videos {[frames[j] for j in eq_a]}")
    for fn in fns.values():
        for _ in range(2): fn()
    times = {k: [] for k in fns}
    for _ in range(int(os.environ.get("ROUNDS", "5"))):
        for k, fn in fns.items():
            torch.cuda.synchronize(); t0 = time.perf_counter()
            for _ in range(steps): fn()
            torch.cuda.synchronize(); times[k].append((time.perf_counter() - t0) / steps)
    for k in fns:
        t = sorted(times[k])
        print(f"{k:8s}: fwd+bwd of all clips median {t[len(t)//2]*1e3:.2f} ms  min {t[0]*1e3:.2f}  max {t[-1]*1e3:.2f}   "
              f"per video {t[len(t)//2]*1e3/len(frames):.2f} ms   (rounds {['%.2f' % (v*1e3) for v in times[k]]})")
    print(f"peak mem {torch.cuda.max_memory_allocated()/2**30:.2f} GiB")
    if os.environ.get("TABLES", "1") != "0":
        for k, fn in fns.items():
            print(f"---- kernel kinds, {k} (per pass over all {len(frames)} clips)")
            kernel_table(fn)
    sys.exit(0)

if os.environ.get("CHUNKS"):
    from memory_augmented_vlm_amd.model import llava_arch as arch
    from memory_augmented_vlm_amd.model.memory_module.MemoryController import BatchedProjector
    counts = sorted((int(v) for v in os.environ["CHUNKS"].split(",")), reverse=True)          # longest first
    vids = [(torch.randn(32 * n, 196, HID, device="cuda") * 0.5).bfloat16() for n in counts]   # distinct videos
    loss_of = lambda mems: sum(cm.float().square().mean() for cm in mems)
    def single_video(v):
        rm.memory_cache = []
        for i in range(v.shape[0] // 32):
            cache, _ = rm(v[32 * i:32 * i + 32])
        return loss_of(cache)
    def singles():
        rm.zero_grad(set_to_none=True)
        sum(single_video(v) for v in vids).backward()
    batches, alone = arch.plan_row_batches(counts)
    bps = {len(g): BatchedProjector(rm, len(g)) for g in batches}
    def grouped():
        rm.zero_grad(set_to_none=True)
        loss = 0.0
        for g in batches:
            bp = bps[len(g)]
            bp.reset()
            for i in range(counts[g[0]]):
                bp.step_train([vids[j][32 * i:32 * i + 32] for j in g])
            loss = loss + sum(loss_of(bp.memory_cache(b)) for b in range(len(g)))
        for j in alone:
            loss = loss + single_video(vids[j])
        loss.backward()
    rbp = BatchedProjector(rm, next(sz for sz in (2, 4, 8) if sz >= len(counts)))
    def ragged():
        rm.zero_grad(set_to_none=True)
        rbp.reset()
        for i in range(counts[0]):
            rbp.step_train([v[32 * i:32 * i + 32] for v, n in zip(vids, counts) if n > i], ragged=True)
        sum(loss_of(rbp.memory_cache(b)) for b in range(len(counts))).backward()
    fns = {"ragged": ragged, "grouped": grouped, "singles": singles}
    print(f"CHUNKS={counts}  M={M} hidden={HID}; equal-length grouping: row batches {[[counts[j] for j in g] for g in batches]}, "
          f"single videos {[counts[j] for j in alone]}")
    for fn in fns.values():
        for _ in range(2): fn()
    times = {k: [] for k in fns}
    for _ in range(int(os.environ.get("ROUNDS", "3"))):
        for k, fn in fns.items():
            torch.cuda.synchronize(); t0 = time.perf_counter()
            for _ in range(steps): fn()
            torch.cuda.synchronize(); times[k].append((time.perf_counter() - t0) / steps)
    for k in fns:
        t = sorted(times[k])
        print(f"{k:8s}: fwd+bwd of all videos median {t[len(t)//2]*1e3:.2f} ms  min {t[0]*1e3:.2f}  max {t[-1]*1e3:.2f}   "
              f"per (video, chunk) step {t[len(t)//2]*1e3/sum(counts):.2f} ms   (rounds {['%.2f' % (v*1e3) for v in times[k]]})")
    print(f"peak mem {torch.cuda.max_memory_allocated()/2**30:.2f} GiB")
    if os.environ.get("TABLES", "1") != "0":
        for k, fn in fns.items():
            print(f"---- kernel kinds, {k} (per pass over all videos: {sum(counts)} (video, chunk) steps, {counts[0]} batch steps)")
            kernel_table(fn)
    sys.exit(0)

if BATCHES != [1]:
    from memory_augmented_vlm_amd.model.memory_module.MemoryController import BatchedProjector
    xs = [x] + [(torch.randn(64, 196, HID, device="cuda") * 0.5).bfloat16() for _ in range(max(BATCHES) - 1)]   # distinct videos
    def batched(B):
        bp = BatchedProjector(rm, B)
        def run():
            rm.zero_grad(set_to_none=True)
            bp.reset()
            for i in range(2):
                bp.step_train([v[32 * i:32 * i + 32] for v in xs[:B]])
            loss = sum(cm.float().square().mean() for b in range(B) for cm in bp.memory_cache(b))
            loss.backward()
        return run
    fns = {B: (step if B == 1 else batched(B)) for B in BATCHES}
    for fn in fns.values():
        for _ in range(2): fn()
    times = {B: [] for B in BATCHES}
    for _ in range(int(os.environ.get("ROUNDS", "3"))):
        for B, fn in fns.items():
            torch.cuda.synchronize(); t0 = time.perf_counter()
            for _ in range(steps): fn()
            torch.cuda.synchronize(); times[B].append((time.perf_counter() - t0) / steps)
    for B in BATCHES:
        t = sorted(times[B])
        print(f"BATCH={B}: train step (fwd+bwd) median {t[len(t)//2]*1e3:.2f} ms  min {t[0]*1e3:.2f}  max {t[-1]*1e3:.2f}   "
              f"per video {t[len(t)//2]*1e3/B:.2f} ms   (M={M} hidden={HID}, rounds {['%.2f' % (v*1e3) for v in times[B]]})")
    print(f"peak mem {torch.cuda.max_memory_allocated()/2**30:.2f} GiB")
    for B in BATCHES:
        print(f"---- kernel kinds, BATCH={B} (ms per step of {B} video(s))")
        kernel_table(fns[B])
    sys.exit(0)

for _ in range(2): step()
torch.cuda.synchronize(); t0 = time.perf_counter()
for _ in range(steps): step()
torch.cuda.synchronize(); dt = (time.perf_counter() - t0) / steps
for _ in range(2): fwd_only()
torch.cuda.synchronize(); t0 = time.perf_counter()
for _ in range(steps): fwd_only()
torch.cuda.synchronize(); df = (time.perf_counter() - t0) / steps
print(f"train step (fwd+bwd) {dt*1e3:.2f} ms   inference fwd {df*1e3:.2f} ms   ratio {dt/df:.2f}   peak mem {torch.cuda.max_memory_allocated()/2**30:.2f} GiB")
lib = capi.lib(); nk = len(capi.KERNEL_KINDS)
ms = (ctypes.c_double * nk)(); ln = (ctypes.c_int64 * nk)(); fl = (ctypes.c_double * nk)(); by = (ctypes.c_double * nk)()
lib.mavlm_prof_enable(1)
for _ in range(steps): step()
torch.cuda.synchronize()
capi.check(lib.mavlm_prof_read(ms, ln, fl, by, nk), "prof"); lib.mavlm_prof_enable(0)
tot = sum(ms)
for i, name in enumerate(capi.KERNEL_KINDS):
    if ln[i]:
        print(f"{name:18s} launches/step {ln[i]/steps:6.1f}  ms/step {ms[i]/steps:8.3f}  ({100*ms[i]/tot:4.1f}%)  avg {ms[i]/ln[i]*1e3:8.1f} us"
              + (f"  {fl[i]/(ms[i]*1e-3)/1e12:7.1f} TF" if fl[i] else f"  {by[i]/(ms[i]*1e-3)/1e9:7.1f} GB/s"))
print(f"sum of HIP kernels {tot/steps:.2f} ms/step (torch glue kernels not included)")
