"""Diagnostic (GPU box): clip row batches - videos of fewer than 32 frames, different frame counts in one step.  Eight clips of
31, 27, 23, 19, 16, 12, 9 and 5 frames at M = 8, hidden 1024 and 896, and four clips (31, 27, 23, 19) at hidden 3584, bf16,
through `run_video_groups` with `clips=True` against `clips=False`.  The switch-off leg runs only code that exists without the
feature (every clip a single video: no two lengths are equal) and is the baseline.  Both legs are warmed up, then alternated in
one process with device synchronisation around every timed window; medians and spread over the rounds, and the launches per pass
by kernel kind (the library's HIP-event brackets), go to profiles/clip_batch.txt.
usage: python tools/diag_clip_batch.py [output file]"""
import ctypes
import os
import sys
import time
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from memory_augmented_vlm_amd import _capi as capi  # noqa: E402

OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "clip_batch.txt")
CASES = ((1024, (31, 27, 23, 19, 16, 12, 9, 5)), (896, (31, 27, 23, 19, 16, 12, 9, 5)), (3584, (31, 27, 23, 19)))
M, P, ROUNDS, REPS = 8, 196, 7, 3
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def median(v):
    return sorted(v)[len(v) // 2]


def launches(fn):
    lib, nk = capi.lib(), len(capi.KERNEL_KINDS)
    ms, ln = (ctypes.c_double * nk)(), (ctypes.c_int64 * nk)()
    fl, by = (ctypes.c_double * nk)(), (ctypes.c_double * nk)()
    lib.mavlm_prof_enable(1)
    fn()
    torch.cuda.synchronize()
    capi.check(lib.mavlm_prof_read(ms, ln, fl, by, nk), "mavlm_prof_read")
    lib.mavlm_prof_enable(0)
    return {name: int(ln[i]) for i, name in enumerate(capi.KERNEL_KINDS) if ln[i]}


def run(dev, hidden, frames):
    model, arch = bench.build_model(dev, hidden=hidden, mem_tokens=M, seed=4321)
    g = torch.Generator(device="cpu").manual_seed(100)
    vids = [(torch.randn((f, P, hidden), generator=g).to(dev).to(torch.bfloat16), torch.arange(f) * 2 + b) for b, f in enumerate(frames)]
    with torch.no_grad():
        mp = model.embed_tokens(torch.tensor(arch.MEMORY_PROMPT_IDS, device=dev)).contiguous()
        fp = model.embed_tokens(torch.tensor(arch.FRAME_PROMPT_IDS, device=dev)).contiguous()

        def leg(on):
            return lambda: arch.run_video_groups(model, vids, mp, fp, model.image_newline, clips=on)

        def timed(fn):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(REPS):
                fn()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) / REPS

        for on in (False, True, False, True):               # warm-up of both legs (engines, workspaces, index caches)
            leg(on)()
        res = {True: [], False: []}
        for _ in range(ROUNDS):
            for on in (True, False):
                res[on].append(timed(leg(on)))
        count = {on: launches(leg(on)) for on in (True, False)}
    m_on, m_off = median(res[True]), median(res[False])
    tot = sum(frames)
    say(f"D={hidden} M={M}: {len(frames)} clips of {frames} frames | clips on {m_on * 1e3:8.4f} ms ({tot / m_on / 1e3:.1f} k frames/s; "
        f"spread {min(res[True]) * 1e3:.4f}-{max(res[True]) * 1e3:.4f}) | off {m_off * 1e3:8.4f} ms ({tot / m_off / 1e3:.1f} k frames/s; "
        f"spread {min(res[False]) * 1e3:.4f}-{max(res[False]) * 1e3:.4f}) | ratio off / on {m_off / m_on:.3f} | "
        f"groups {arch.plan_clip_batches(list(frames))}")
    for on in (True, False):
        say(f"    launches per pass, clips {'on ' if on else 'off'}: {sum(count[on].values())} = {count[on]}")


def main():
    if not torch.cuda.is_available():
        lines.append("tools/diag_clip_batch.py: not measured (no GPU in this run)")
    else:
        dev = torch.device("cuda", 0)
        torch.cuda.set_device(dev)
        say(f"tools/diag_clip_batch.py: medians of {ROUNDS} alternated rounds of {REPS} passes, bf16, {torch.cuda.get_device_name(0)}")
        for hidden, frames in CASES:
            try:
                run(dev, hidden, frames)
            except capi.MavlmError as e:          # (a width the kernels refuse is reported, not hidden)
                say(f"D={hidden} M={M}: not run - {e}")
    os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
    with open(OUT, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
