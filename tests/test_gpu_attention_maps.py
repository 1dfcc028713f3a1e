"""-m gpu: attention maps - the mass of the softmax probabilities per (head, query group, key group) cell.

  mass[h, i, j] = sum over q in query group i, k in key group j of p[h, q, k]          (attention_maps.hip)

Operator against float64 (a true softmax of the same 16-bit operands: it never sees the GPU's lse2), size-independent
properties, the fused step's maps against the operator's definition on the step's own Q / K, "recording changes nothing else",
and the reference's grouped probabilities (golden/g10_attention_maps.npz).

Plain normal Q and K give an almost uniform map (a group sum averages tens of thousands of probabilities), which a kernel that
ignores its data would nearly reproduce.  Every comparison therefore runs on inputs with one offset row per group and first
asserts, on the EXPECTATION, a relative distance of at least 0.1 from the uniform map rows_i * keys_j / S."""
import ctypes
import math

import numpy as np
import pytest
import torch

import memory_augmented_vlm_amd  # noqa: F401
from memory_augmented_vlm_amd import _capi as capi
from memory_augmented_vlm_amd import _ops as ops
from memory_augmented_vlm_amd.model.memory_module.MemoryController import BatchedProjector, FusedAttentionStats
from oracle import memory_path as O
from conftest import load_golden
from gpu_util import to_dev, to_np

pytestmark = pytest.mark.gpu
TOL = 1e-3              # the single-stage gate of tests/test_gpu_ops.py (the column-sum pass is held to it)
MIN_FROM_UNIFORM = 0.1
P = 196


def _grouped_inputs(R, S, W, qg, kg, mode, seed):
    """normal Q [R, W], K [S, W] plus one unit-scale offset row per query group / key group, rounded to the 16-bit grid"""
    q = O.hash_normal_like((R, W), seed)
    k = O.hash_normal_like((S, W), seed + 1)
    q = q + O.hash_normal_like((-(-R // qg), W), seed + 2)[np.arange(R) // qg]
    k = k + O.hash_normal_like((-(-S // kg), W), seed + 3)[np.arange(S) // kg]
    r = O.rounder(mode)
    return r(q), r(k)


def _uniform(R, S, H, qg, kg):
    rows = np.minimum(qg, R - np.arange(-(-R // qg)) * qg).astype(np.float64)
    keys = np.minimum(kg, S - np.arange(-(-S // kg)) * kg).astype(np.float64)
    return np.broadcast_to(rows[:, None] * keys[None, :] / S, (H, rows.size, keys.size))


def _group_sum(x, g, axis):
    """sums of consecutive groups of g along `axis` (last group may be short); numpy or torch"""
    n = x.shape[axis]
    pad = -(-n // g) * g - n
    if isinstance(x, torch.Tensor):
        x = torch.movedim(x, axis, -1)
        x = torch.nn.functional.pad(x, (0, pad))
        return torch.movedim(x.reshape(x.shape[:-1] + (-1, g)).sum(-1), -1, axis)
    x = np.moveaxis(x, axis, -1)
    x = np.concatenate([x, np.zeros(x.shape[:-1] + (pad,), dtype=x.dtype)], axis=-1)
    return np.moveaxis(x.reshape(x.shape[:-1] + (-1, g)).sum(-1), -1, axis)


def mass_ref64_np(q, k, H, hd, scale, qg, kg):
    """the definition in numpy float64: true softmax per head, grouped sums"""
    q, k = np.asarray(q, dtype=np.float64), np.asarray(k, dtype=np.float64)
    out = []
    for h in range(H):
        s = (q[:, h * hd:(h + 1) * hd] @ k[:, h * hd:(h + 1) * hd].T) * scale
        p = np.exp(s - s.max(axis=1, keepdims=True))
        p /= p.sum(axis=1, keepdims=True)
        out.append(_group_sum(_group_sum(p, kg, 1), qg, 0))
    return np.stack(out)


def mass_ref64_torch(q, k, H, hd, scale, qg, kg, width=None):
    """the same in torch float64 on the operands' device (a query group at a time would be slow: blocks of whole groups).
    `width`: column stride between heads (zero-padded heads: 128), default hd"""
    width = width or hd
    R = q.shape[0]
    rows = max(qg, (2048 // qg) * qg)
    out = []
    for h in range(H):
        kh = k[:, h * width:h * width + hd].double()
        acc = []
        for r0 in range(0, R, rows):
            s = (q[r0:r0 + rows, h * width:h * width + hd].double() @ kh.T) * scale
            p = torch.softmax(s, dim=1)
            acc.append(_group_sum(_group_sum(p, kg, 1), qg, 0))
        out.append(torch.cat(acc, dim=0))
    return torch.stack(out)


def _check_operator(q, k, H, hd, qg, kg, mode, exp, label):
    """`exp`: float64 expectation (numpy).  Gates: distance from uniform on the expectation, rel-L2 against it, row sums,
    column sums against the column-sum pass, same bits on a second call."""
    R, S = q.shape[0], k.shape[0]
    far = O.rel_l2(exp, _uniform(R, S, H, qg, kg))
    assert far >= MIN_FROM_UNIFORM, (label, far)
    dq, dk = to_dev(q, mode), to_dev(k, mode)
    _, lse = ops.attention(dq, dk, dk, H, want_lse=True, head_dim=hd)
    got = ops.attention_group_mass(dq, dk, lse, H, qg, kg, head_dim=hd)
    assert tuple(got.shape) == (H, -(-R // qg), -(-S // kg)) and got.dtype == torch.float32
    err = O.rel_l2(to_np(got.double()), exp)
    rows = np.minimum(qg, R - np.arange(-(-R // qg)) * qg).astype(np.float64)
    rowsum = to_np(got.double().sum(-1))
    rs_err = float(np.max(np.abs(rowsum - rows[None, :]) / rows[None, :]))
    col = ops.attention_colsum(dq, dk, lse, H, head_dim=hd)
    col_err = O.rel_l2(to_np(got.double().sum(1)), to_np(_group_sum(col.double(), kg, 1)))
    print(f"group_mass {label} {mode}: rel-L2 vs fp64 {err:.2e}, row sums {rs_err:.2e}, vs column-sum pass {col_err:.2e}, "
          f"expectation {far:.2f} from uniform")
    assert err < TOL, (label, err)
    assert rs_err < 1e-3, (label, rs_err)
    assert col_err < TOL, (label, col_err)
    assert torch.equal(ops.attention_group_mass(dq, dk, lse, H, qg, kg, head_dim=hd), got)
    return got


# ------------------------------------------------------------------------------------------------------------------ operator
CASES = [(1568, 6272, 8, 128, 196, 196), (1568, 6272, 8, 128, 100, 400), (1568, 6272, 8, 128, 196, 1568),
         (300, 2000, 2, 128, 196, 196), (300, 2000, 2, 128, 100, 400), (196, 64 * 40 + 17, 4, 128, 28, 196),
         (1568, 6272, 8, 448, 196, 196), (1500, 700, 3, 448, 196, 196)]


@pytest.mark.parametrize("mode", ["bf16", "fp16"])
@pytest.mark.parametrize("R,S,H,hd,qg,kg", CASES, ids=lambda v: str(v))
def test_group_mass_vs_fp64(mode, R, S, H, hd, qg, kg):
    q, k = _grouped_inputs(R, S, H * hd, qg, kg, mode, 300 + hd)
    exp = mass_ref64_np(q, k, H, hd, 1.0 / math.sqrt(hd), qg, kg)
    _check_operator(q, k, H, hd, qg, kg, mode, exp, f"R{R} S{S} H{H} hd{hd} groups({qg},{kg})")


@pytest.mark.parametrize("mode,kg", [("bf16", 196), ("fp16", 1568)])
def test_group_mass_64_memory_tokens_vs_fp64_on_device(mode, kg):
    """R = 64 x 196 rows against a 32-frame chunk, expectation in torch float64 on the GPU"""
    R, S, H, hd, qg = 12544, 6272, 8, 128, 196
    q, k = _grouped_inputs(R, S, H * hd, qg, kg, mode, 411)
    exp = mass_ref64_torch(to_dev(q, mode), to_dev(k, mode), H, hd, 1.0 / math.sqrt(hd), qg, kg)
    _check_operator(q, k, H, hd, qg, kg, mode, exp.cpu().numpy(), f"R{R} S{S} H{H} hd{hd} groups({qg},{kg})")


def test_group_mass_reads_column_slices_and_a_scale():
    """operands that are column slices of wider buffers (as the step's K inside the packed K/V buffer), an explicit scale"""
    R, S, H, hd, qg, kg = 392, 980, 2, 128, 196, 196
    q, k = _grouped_inputs(R, S, H * hd, qg, kg, "bf16", 77)
    wide = torch.zeros((S, 3 * H * hd), device="cuda", dtype=torch.bfloat16)
    wide[:, H * hd:2 * H * hd] = to_dev(k, "bf16")
    dq, dk = to_dev(q, "bf16"), wide[:, H * hd:2 * H * hd]
    scale = 0.07
    _, lse = ops.attention(dq, dk, dk, H, want_lse=True, scale=scale)
    got = ops.attention_group_mass(dq, dk, lse, H, qg, kg, scale=scale)
    exp = mass_ref64_np(q, k, H, hd, scale, qg, kg)
    assert O.rel_l2(exp, _uniform(R, S, H, qg, kg)) >= MIN_FROM_UNIFORM
    assert O.rel_l2(to_np(got.double()), exp) < TOL
    st = FusedAttentionStats(dq, dk, lse, H)
    assert tuple(st.group_mass(qg, kg).shape) == (H, 2, 5)


# ---------------------------------------------------------------------------------------------------------------- fused step
@pytest.fixture()
def no_grad():
    with torch.no_grad():
        yield


def _offset_frames(f, D, seed, amp=1.0):
    """chunk frames: normal patches + one normal offset vector per frame (the condition that keeps the maps away from uniform)"""
    return O.bf16_round(O.hash_normal_like((f, P, D), seed) + amp * O.hash_normal_like((f, 1, D), seed + 100))


def _step_operands(eng, F, b=0):
    """Q [R, Dp], K [S, Dp] (last formation layer) and lse2 [H, R] the last step of video b left in the workspace"""
    c = eng.c
    B, R, S, L, H, Dp = max(eng.batch, 1), c.mem_tokens * c.patches, F * c.patches, c.depth, c.heads, eng.Dp
    offs = (ctypes.c_size_t * 10)()
    capi.check(capi.lib().mavlm_workspace_layout(c, offs, 10), "mavlm_workspace_layout")
    assert capi.lib().mavlm_prefetch_hits(eng.ctx) == 0          # the step read the first chunk K/V buffer (entry 0)

    def view(o, n, dt):
        b0 = eng.workspace_base_offset + o
        return eng.workspace[b0:b0 + n * (4 if dt == torch.float32 else 2)].view(dt)

    q = view(offs[1], B * R * Dp, eng.dtype).view(B, R, Dp)[b]
    kv = view(offs[0], B * S * 2 * L * Dp, eng.dtype).view(B, S, 2 * L * Dp)[b]
    lse = view(offs[8], B * H * R, torch.float32).view(B, H, R)[b]
    return q, kv[:, 2 * (L - 1) * Dp:(2 * L - 1) * Dp], lse


def _gate_step_maps(eng, maps, scores, F, n_past, mode, label, b=0):
    """check 4 for the maps of one step of video b: the last formation layer against float64 of the step's own Q / K, row sums of
    every map, column sums of the last layer against the column-sum pass, and the frame scores"""
    c = eng.c
    H, M, L = c.heads, c.mem_tokens, c.depth
    hd = c.hidden // H
    hdw = hd if hd > 128 else 128
    form, evo = maps.formation, maps.evolution
    assert tuple(form.shape) == (L, H, M, F) and form.dtype == torch.float32
    q, k, lse = _step_operands(eng, F, b)
    scale = ops.attn_scale(hd)
    exp = mass_ref64_torch(q, k, H, hd, scale, P, P, width=hdw)
    far = float(torch.linalg.vector_norm(exp - P / F) / torch.linalg.vector_norm(torch.full_like(exp, P / F)))
    assert far >= MIN_FROM_UNIFORM, (label, far)
    err = float(torch.linalg.vector_norm(form[-1].double() - exp) / torch.linalg.vector_norm(exp))
    rs = float((form.double().sum(-1) - P).abs().max() / P)
    col = ops.attention_colsum(q, k, lse, H, head_dim=hdw, scale=scale)
    col_err = O.rel_l2(to_np(form[-1].double().sum(1)), to_np(_group_sum(col.double(), P, 1)))
    fs = form[-1].double().sum(dim=(0, 1)) / P
    fs_err = O.rel_l2(to_np(scores.double()), to_np(fs))
    fs_tol = TOL + 2.0 ** (-9 if mode == "bf16" else -12)      # + the rounding of the stored 16-bit scores (half an ulp)
    msg = (f"step maps {label}: last layer vs fp64 {err:.2e} ({far:.2f} from uniform), row sums {rs:.2e}, vs column-sum pass "
           f"{col_err:.2e}, frame scores {fs_err:.2e} (gate {fs_tol:.2e})")
    if n_past:
        assert tuple(evo.shape) == (H, M, n_past)
        ers = float((evo.double().sum(-1) - P).abs().max() / P)
        msg += f", evolution row sums {ers:.2e}"
        assert ers < 1e-3, (label, ers)
    else:
        assert evo is None
    print(msg)
    assert err < TOL and rs < 1e-3 and col_err < TOL and fs_err < fs_tol, msg


@pytest.mark.parametrize("D,mode", [(1024, "bf16"), (3584, "bf16"), (1024, "fp16")])
def test_step_maps_vs_fp64_of_the_steps_operands(D, mode, no_grad):
    """one video of two 32-frame chunks and a short one, M = 8: after every step the maps against float64 of that step's Q / K"""
    from test_gpu_path import make_projector
    cfg = O.PathConfig(hidden=D, heads=8, mem_tokens=8, depth=2)
    proj = make_projector(cfg, O.make_weights(cfg, seed=1601), mode)
    proj.record_attention_maps = True
    proj.memory_cache = []
    for t, f in enumerate((32, 32, 5)):
        seg = to_dev(_offset_frames(f, D, 1610 + t), mode)
        _, scores = proj(seg)
        assert len(proj.attention_maps) == t + 1
        _gate_step_maps(proj._engine, proj.attention_maps[-1], scores[-1], f, t, mode, f"D{D} {mode} chunk {t}")
    proj.memory_cache = []
    assert proj.attention_maps == []


def test_evolution_map_is_ordered_oldest_first_after_the_ring_wraps(no_grad):
    """cache_cap 3, 5 steps: the evolution map's columns follow torch.cat(memory_cache) (oldest first), not the ring's slots.
    Expectation: float64 of the definition on the projections of the cached memories in FIFO order.  The order only shows where
    the columns differ: the expectation must sit at least 10 x TOL from uniform, so that a permuted map misses the gate."""
    from test_gpu_path import make_projector
    D, H, M, cap = 256, 2, 2, 3
    cfg = O.PathConfig(hidden=D, heads=H, mem_tokens=M, depth=1)
    proj = make_projector(cfg, O.make_weights(cfg, seed=1650), "bf16", cache_cap=cap)
    proj.record_attention_maps = True
    proj.memory_cache = []
    att = proj.memory_update_attention
    prev = None                                   # the FIFO the step's evolution attends over (oldest first)
    for t in range(5):
        cache, _ = proj(to_dev(_offset_frames(2, D, 1660 + t)))
        evo = proj.attention_maps[-1].evolution
        if prev is None:
            assert evo is None
        else:
            # (the step's own Q was overwritten by the formation layer: the same projections through the operator)
            q = ops.linear(prev[-1].reshape(M * P, D), att.q_proj.weight, att.q_proj.bias.float())
            keys = torch.cat([ops.linear(m_.reshape(M * P, D), att.k_proj.weight, att.k_proj.bias.float()) for m_ in prev])
            exp = mass_ref64_torch(q, keys, H, D // H, ops.attn_scale(D // H), P, M * P)
            far = float(torch.linalg.vector_norm(exp - P / len(prev)) / torch.linalg.vector_norm(torch.full_like(exp, P / len(prev))))
            err = float(torch.linalg.vector_norm(evo.double() - exp) / torch.linalg.vector_norm(exp))
            print(f"evolution map, step {t} ({len(prev)} cached): vs fp64 in FIFO order {err:.2e}, {far:.3f} from uniform")
            assert tuple(evo.shape) == (H, M, len(prev)) and err < TOL
            if t >= cap:                          # the ring has wrapped: slot order != age order
                assert far >= 10 * TOL, far
        prev = [c.clone() for c in cache]
    assert len(prev) == cap


@pytest.mark.parametrize("M", [8])
def test_recording_changes_nothing_else(M, no_grad):
    """flag off (eager, captured, replayed) and on: memory ring, frame scores and the emitted tokens are the same bits; with the
    flag on `_video_tokens` runs eagerly and fills `attention_maps`, and a replay afterwards still works"""
    from test_gpu_path import _tiny_host
    from memory_augmented_vlm_amd.model import llava_arch as arch
    D, T = 1024, 40

    class LM(arch.LlavaMetaForCausalLM):
        def __init__(self, model):
            self.model = model

        def get_model(self):
            return self.model

    cfg = O.PathConfig(hidden=D, heads=8, mem_tokens=M, depth=2)
    model, _ = _tiny_host(cfg, O.make_weights(cfg, seed=1701))
    lm = LM(model)
    lm.enable_memory_graphs(2)
    rm = model.recurrent_memory_transformer
    x = to_dev(_offset_frames(T, D, 1710))
    idx = torch.arange(T)
    g = torch.Generator(device="cpu").manual_seed(5)
    mp, fp = torch.randn((10, D), generator=g).to("cuda").bfloat16(), torch.randn((9, D), generator=g).to("cuda").bfloat16()

    def run():
        rm.frame_attn_scores = []
        out = lm._video_tokens(model, x, idx, mp, fp, True).clone()
        return out, [c.clone() for c in rm.memory_cache], [s.clone() for s in rm.frame_attn_scores]

    off = run()                                   # eager
    assert rm.attention_maps == []
    run()                                         # captures
    assert len(lm._mem_graphs) == 1
    replay = run()
    rm.record_attention_maps = True
    on = run()
    assert len(rm.attention_maps) == 2 and rm.attention_maps[0].evolution is None
    assert tuple(rm.attention_maps[1].evolution.shape) == (8, M, 1) and tuple(rm.attention_maps[1].formation.shape) == (2, 8, M, 8)
    rm.record_attention_maps = False
    again = run()
    for other in (replay, on, again):
        assert torch.equal(off[0], other[0])
        assert len(other[1]) == len(off[1]) and all(torch.equal(a, b) for a, b in zip(off[1], other[1]))
    assert len(on[2]) == len(off[2]) == 2 and all(torch.equal(a, b) for a, b in zip(off[2], on[2]))


def test_row_batch_maps(no_grad):
    """a row batch of two different videos: each video's maps pass the single video's gates, and recording leaves the batch's
    memories and scores the same bits"""
    from test_gpu_path import make_projector
    D, mode = 1024, "bf16"
    cfg = O.PathConfig(hidden=D, heads=8, mem_tokens=8, depth=2)
    proj = make_projector(cfg, O.make_weights(cfg, seed=1801), mode)
    vids = [[to_dev(_offset_frames(f, D, 1810 + 10 * b + t), mode) for t, f in enumerate((32, 6))] for b in range(2)]
    keep = {}
    for record in (False, True):
        bp = BatchedProjector(proj, 2)
        bp.record_attention_maps = record
        bp.reset()
        for t in range(2):
            scores = bp.step([vids[0][t], vids[1][t]])
            if record:
                am = bp.attention_maps[-1]
                assert am.formation.shape[0] == 2
                for b in range(2):
                    one = type(am)(am.formation[b], am.evolution[b] if am.evolution is not None else None)
                    _gate_step_maps(bp._engine, one, scores[b], vids[b][t].shape[0], t, mode, f"row batch video {b} chunk {t}", b)
        torch.cuda.synchronize()
        keep[record] = ([torch.stack(bp.memory_cache(b)).clone() for b in range(2)], [s.clone() for s in bp.frame_scores])
        assert len(bp.attention_maps) == (2 if record else 0)
    assert all(torch.equal(a, b) for a, b in zip(keep[False][0], keep[True][0]))
    assert all(torch.equal(a, b) for a, b in zip(keep[False][1], keep[True][1]))
    assert not torch.equal(keep[True][0][0], keep[True][0][1])


def test_autograd_path_refuses_the_flag():
    from test_gpu_path import make_projector
    cfg = O.PathConfig(hidden=256, heads=2, mem_tokens=2, depth=1)
    proj = make_projector(cfg, O.make_weights(cfg, seed=1901))
    proj.record_attention_maps = True
    proj.memory_cache = []
    with torch.enable_grad(), pytest.raises(capi.MavlmError, match="record_attention_maps.*autograd"):
        proj(to_dev(_offset_frames(1, 256, 1902)))


# ------------------------------------------------------------------------------------------------------------- the reference
def test_maps_vs_reference_golden(no_grad):
    """The reference projector's grouped probabilities (golden/g10_attention_maps.npz, D = 1024, H = 8, M = 8, depth 2, chunks of
    32, 32 and 7 frames).  The GPU's bf16 maps against the reference's fp32 maps, per map; the yardstick is the reference's own
    envelope e = rel_l2(reference bf16, reference fp32) from the fixture: gate max(2 e, 1e-3) - twice, because two correct
    16-bit chains decorrelate at every storage rounding (chain_tol, tests/test_gpu_path.py), never below the single-stage gate."""
    from test_gpu_path import make_projector
    z, meta = load_golden("g10_attention_maps.npz")
    cfg = O.PathConfig(hidden=meta["hidden"], heads=meta["heads"], mem_tokens=meta["mem_tokens"], depth=meta["depth"])
    proj = make_projector(cfg, O.make_weights(cfg, seed=meta["wseed"]), "bf16")
    proj.record_attention_maps = True
    proj.memory_cache = []
    rows, bad = [], []
    for t, f in enumerate(meta["frames"]):
        x = O.bf16_round(O.hash_normal_like((f, P, cfg.hidden), meta["segseed0"] + t)
                         + meta["amplitude"] * O.hash_normal_like((f, 1, cfg.hidden), meta["offseed0"] + t))
        proj(to_dev(x))
        am = proj.attention_maps[-1]
        for l in range(cfg.depth):
            e = meta["envelope_formation"][t][l]
            err = O.rel_l2(to_np(am.formation[l]), z[f"fp32_form_{t}"][l])
            rows.append((f"chunk {t} formation layer {l}", err, e))
        if t:
            e = meta["envelope_evolution"][t - 1]
            rows.append((f"chunk {t} evolution", O.rel_l2(to_np(am.evolution), z[f"fp32_evo_{t}"]), e))
    for name, err, e in rows:
        gate = max(2.0 * e, TOL)
        print(f"{name}: GPU bf16 vs reference fp32 {err:.2e}; reference bf16 vs fp32 {e:.2e}; gate {gate:.2e}")
        if not err < gate:
            bad.append((name, err, gate))
    assert not bad, bad
