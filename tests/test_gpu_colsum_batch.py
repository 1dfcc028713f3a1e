"""-m gpu: the row-batched column-sum pass (`mavlm_attention_colsum_batch`, `ops.attention_colsum_batch`) - the frame scores of
a row batch's training step in one launch.

Every video carries its own data.  K is a column slice of one wider buffer whose rows BETWEEN two videos hold 3e4 (one of them
read as a key cannot go unnoticed); Q and lse2 are stacked, so a ragged last Q tile that reached past its video would read the
next video's rows.  `part` is filled with a sentinel before the launch: what lies behind each video's planes must stay intact.
Yardsticks: nb launches of the single-video operator (bit for bit: same schedule per video, no atomics) and the float64 column
sums of the softmax of the same Q, K in numpy at the operator gate 1e-3 (that of tests/test_gpu_batch_train.py, restated)."""
import numpy as np
import pytest
import torch

import memory_augmented_vlm_amd  # noqa: F401
from memory_augmented_vlm_amd import _capi as capi
from memory_augmented_vlm_amd import _ops as ops
from oracle import memory_path as O
from gpu_util import to_dev, to_np, DT

pytestmark = pytest.mark.gpu
OP_TOL = 1e-3
BIG = 3.0e4
SENTINEL = -7.25


def _plan(R, S, H):
    info = (capi.C.c_int32 * 2)()
    capi.check(capi.lib().mavlm_attention_colsum_plan(R, S, H, info), "mavlm_attention_colsum_plan")
    return info[0], info[1]


def _case(mode, hw, nb, H, R, S, seed):
    r = O.rounder(mode)
    W = H * hw
    gap = 5
    Q = r(O.hash_normal_like((nb * R, W), seed, 1.0))
    K = r(O.hash_normal_like((nb, S, W), seed + 1, 1.0))
    buf = torch.full((nb, S + gap, W + 64), BIG, device="cuda", dtype=DT[mode])
    buf[:, :S, 32:32 + W] = to_dev(K, mode)
    k = buf[:, :S, 32:32 + W]
    assert k.stride(0) > S * k.stride(1)
    return Q, K, to_dev(Q, mode), k


def _float64_colsum(Q, K, H, hw, scale):
    """[H, S]: column sums over the queries of softmax(scale * Q_h K_h^T), float64"""
    out = []
    for h in range(H):
        q, k = Q[:, h * hw:(h + 1) * hw].astype(np.float64), K[:, h * hw:(h + 1) * hw].astype(np.float64)
        s = scale * (q @ k.T)
        p = np.exp(s - s.max(axis=1, keepdims=True))
        out.append((p / p.sum(axis=1, keepdims=True)).sum(axis=0))
    return np.stack(out)


def _check(mode, hw, nb, H, R, S, seed, want_planes=False):
    Q, K, q, k = _case(mode, hw, nb, H, R, S, seed)
    scale = ops.attn_scale(hw)
    lib = capi.lib()
    # the forward's lse2, per video (never-split grid), stacked [nb*H, R] as the batched forward writes it
    lse = []
    v = torch.zeros_like(k)
    for b in range(nb):
        kw = dict(plain=True) if hw == 128 else dict(head_dim=hw)
        lse.append(ops.attention(q[b * R:(b + 1) * R], k[b], v[b], H, want_lse=True, scale=scale, **kw)[1])
    lse = torch.cat(lse).contiguous()
    single = torch.stack([ops.attention_colsum(q[b * R:(b + 1) * R], k[b], lse[b * H:(b + 1) * H], H, head_dim=hw, scale=scale)
                          for b in range(nb)])
    planes = _plan(R, S, H)[1] if hw == 128 else 1
    if want_planes:
        assert planes > 1, (R, S, H, planes)
    per = int(lib.mavlm_attention_colsum_floats(R, S, H))
    assert int(lib.mavlm_attention_colsum_batch_floats(R, S, H, nb)) == nb * per and per >= planes * H * S
    tail = 64
    buf = torch.full((nb * per + tail,), SENTINEL, device="cuda", dtype=torch.float32)
    capi.check(lib.mavlm_attention_colsum_batch(q.data_ptr(), q.stride(0), k.data_ptr(), k.stride(1), k.stride(0), lse.data_ptr(),
                                                buf.data_ptr(), nb * per, R, S, H, nb, hw, scale, ops.dtype_code(q.dtype),
                                                ops.stream_ptr()), "mavlm_attention_colsum_batch")
    torch.cuda.synchronize()
    body = buf[:nb * per].view(nb, per)
    got = body[:, :H * S].view(nb, H, S)
    assert torch.equal(got, single), "batched column sums differ from per-video launches"
    assert bool((body[:, planes * H * S:] == SENTINEL).all()), "written behind a video's planes"
    assert bool((buf[nb * per:] == SENTINEL).all()), "written behind the buffer"
    # the Python operator: the same launch into its own buffer
    part = ops.attention_colsum_batch(q, k, lse, H, nb, head_dim=hw, scale=scale)
    assert tuple(part.shape) == (nb, H, S) and part.dtype == torch.float32 and torch.equal(part, single)
    for b in range(nb):
        ref = _float64_colsum(Q[b * R:(b + 1) * R], K[b], H, hw, scale)
        err = O.rel_l2(to_np(part[b]), ref)
        print(f"head {hw} {mode} R {R} S {S} video {b}: column sums rel-L2 vs float64 {err:.2e} (planes {planes})")
        assert err < OP_TOL, (b, err)


@pytest.mark.parametrize("mode", ["bf16", "fp16"])
def test_batched_colsum_equals_per_video_launches_head_128(mode):
    """nb = 3 videos of 2 heads, R = 200 (ragged against the 64-row Q tiles: the last tile of videos 0 and 1 ends inside the
    next video's rows), S = 260 (ragged against the 128-key blocks)"""
    _check(mode, 128, 3, 2, 200, 260, 5100)


@pytest.mark.parametrize("mode", ["bf16", "fp16"])
def test_batched_colsum_equals_per_video_launches_head_448(mode):
    """the wide heads: nb = 2, 2 heads, R = 100 (ragged against the 32-row tiles), S = 150"""
    _check(mode, 448, 2, 2, 100, 150, 5200)


# smallest R (S = 784, 2 heads) at which a (key block, head) unit's query tiles are spread over more than one workgroup, i.e.
# the pass writes several planes per video and the batched plane reduction runs: 14 units, so the schedule cuts units as soon as
# ttot / 8 > 14, i.e. from 9 query tiles of 64 on
MULTI_PLANE = dict(R=513, S=784, H=2)


def test_batched_colsum_several_planes():
    s = MULTI_PLANE
    assert _plan(s["R"], s["S"], s["H"])[1] > 1 and _plan(s["R"] - 1, s["S"], s["H"])[1] == 1
    _check("bf16", 128, 2, s["H"], s["R"], s["S"], 5300, want_planes=True)
