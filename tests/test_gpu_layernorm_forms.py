"""-m gpu: every form of the row LayerNorm, forward and backward, against torch float64.

Forward (csrc/elementwise.hip `ln_dispatch`): the widths of tests/layernorm_cases.py - held to the dispatch itself on the CPU by
tests/test_layernorm_forms_cpu.py - reach `layernorm8_kernel<T, 1 / 2 / 4>`, `layernorm8_block_kernel<T, 2>` and the 4-element
fallback `layernorm_kernel<T, 1 .. 16>`, each at its narrowest and widest row, at a partly filled last chunk row and at rows = 1,
in bf16 and fp16, without and with a 16-bit residual (the fallback also through a residual whose row stride is 4 mod 8).  Every
call writes through `out=` into the middle of a buffer filled with a sentinel, is made twice and must repeat bit for bit; the
rows before and behind the output keep the sentinel.

Inputs: the rows of test_gpu_ops.py::test_layernorm_vs_oracle (x = 3 N(0,1) + 0.5, gamma 1 +- 0.1, beta +- 0.1); rows of
x = 64 + N(0,1), whose mean is 64 standard deviations out - they keep the variance two-pass (E[x^2] - E[x]^2 in fp32 would lose
it) and show a chunk dropped from a sum at any width (tests/test_gates_cpu.py); constant rows, which must give beta rounded,
exactly.

The reference is torch float64 on the GPU from the same operands; the gate is `gpu_util.layernorm_gate`: per block of 4 rows
(the rows of one workgroup of the wave-per-row forms) within BWD_BLOCK x the floor of the reference rounded once to the output
grid.  The kernels compute in fp32 and round once, so the expected ratio is 1.0; the worst ratio per form is printed (-s) and
tabulated in tests/README.md.

Backward (csrc/backward.hip `launch_ln_bwd`): NV = 2 and 8, and D = 4096 (96 KiB of dynamic LDS), with the gates of
test_gpu_backward_m64.py::test_layernorm_bwd_m64_vs_fp64 unchanged."""
import pytest
import torch

import memory_augmented_vlm_amd  # noqa: F401
from memory_augmented_vlm_amd import _capi as capi
from memory_augmented_vlm_amd import _ops as ops
from gpu_util import BWD_BLOCK, DT, f32_sum_gate, floor_gate, layernorm_gate, layernorm_ref64
import layernorm_cases as L

pytestmark = pytest.mark.gpu
SENTINEL = -1234.0              # on both 16-bit grids; no LayerNorm output of these inputs comes near it
WORST = {}                      # form name -> worst measured ratio (printed as the cases run)


def _randn(shape, seed, std=1.0, mean=0.0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return torch.randn(shape, generator=g, device="cuda") * std + mean


def _twice(x, gamma, beta, eps, mode, res):
    """ops.layernorm through out=, twice, each time into rows [1, rows] of a sentinel-filled [rows + 2, D] buffer: the same
    bits, and the guard rows untouched."""
    rows, d = x.shape
    outs = []
    for _ in range(2):
        buf = torch.full((rows + 2, d), SENTINEL, device="cuda", dtype=DT[mode])
        got = ops.layernorm(x, gamma, beta, eps, DT[mode], out=buf[1:rows + 1], residual=res)
        assert got.data_ptr() == buf[1].data_ptr()
        assert bool((buf[0] == SENTINEL).all()) and bool((buf[rows + 1] == SENTINEL).all())
        outs.append(buf[1:rows + 1])
    assert torch.equal(outs[0], outs[1])
    return outs[0]


def _residual(rows, d, ldr, seed, mode):
    """16-bit [rows, d] residual of row stride ldr: a [:, :d] view of a [rows, ldr] tensor where ldr > d"""
    full = _randn((rows, ldr), seed).to(DT[mode])
    res = full[:, :d]
    assert res.stride(0) == ldr
    return res


_FWD = [pytest.param(form, d, ldr, mode, rows, 1e-12, id=f"{L.form_name(form)}-D{d}" + (f"-ldr{ldr}" if ldr != d else "") + f"-{mode}-rows{rows}")
        for form, d, ldr in L.FORWARD_CASES for mode in ("bf16", "fp16") for rows in (1, 37)] + \
       [pytest.param(L.LN8 + 4, 1152, 1152, "bf16", 37, 1e-5, id="ln8-nc4-D1152-bf16-rows37-eps1e-5")]


@pytest.mark.parametrize("form,d,ldr,mode,rows,eps", _FWD)
def test_layernorm_forward_form_vs_fp64(form, d, ldr, mode, rows, eps):
    assert capi.lib().mavlm_layernorm_form(d, ldr) == form
    gamma = 1.0 + (torch.rand(d, generator=torch.Generator(device="cuda").manual_seed(52), device="cuda") - 0.5) * 0.2
    beta = (torch.rand(d, generator=torch.Generator(device="cuda").manual_seed(53), device="cuda") - 0.5) * 0.2
    res = _residual(rows, d, ldr, 54, mode)
    inputs = {"3N+0.5": _randn((rows, d), 51, 3.0, 0.5), "64+N": _randn((rows, d), 55, 1.0, 64.0)}
    gates = []
    for kind, x in inputs.items():
        for r in (None, res):                 # (without a residual the two widths over a wider stride run their ln8 / block form)
            got = _twice(x, gamma, beta, eps, mode, r)
            gates.append(layernorm_gate(f"{kind} {'residual' if r is not None else 'no residual'}", got,
                                        layernorm_ref64(x, r, gamma, beta, eps), mode))
    worst = max(g.worst for g in gates)
    name = L.form_name(form)
    WORST[name] = max(WORST.get(name, 0.0), worst)
    print(f"\n[layernorm {name} D={d} ldr={ldr} {mode} rows={rows} eps={eps}] worst block {worst:.4f} x floor "
          f"(form so far {WORST[name]:.4f})\n  " + "\n  ".join(str(g) for g in gates))
    assert all(g.ok for g in gates), [str(g) for g in gates if not g.ok]
    # constant rows: var = 0 -> rsqrt(0 + eps) finite, every element minus the mean exactly 0: the output is beta, rounded
    want = beta.to(DT[mode]).expand(rows, d)
    xc = torch.full((rows, d), 2.5, device="cuda")
    assert torch.equal(_twice(xc, gamma, beta, eps, mode, None), want)
    rc = torch.full((rows, ldr), 0.5, device="cuda", dtype=DT[mode])[:, :d]
    assert torch.equal(_twice(xc, gamma, beta, eps, mode, rc), want)


@pytest.mark.parametrize("mode", ["bf16", "fp16"])
@pytest.mark.parametrize("form,d,ldr", L.REFUSED_CASES, ids=[f"D{d}" for _, d, _ in L.REFUSED_CASES])
def test_layernorm_forward_refusals_write_nothing(form, d, ldr, mode):
    """More than 4096 columns, or a width off the 4-element grid: MavlmError before anything is enqueued."""
    rows = 5
    assert capi.lib().mavlm_layernorm_form(d, ldr) == L.REFUSED
    x = _randn((rows, d), 61)
    gamma, beta = torch.ones(d, device="cuda"), torch.zeros(d, device="cuda")
    for res in (None, _randn((rows, d), 62).to(DT[mode])):
        buf = torch.full((rows, d), SENTINEL, device="cuda", dtype=DT[mode])
        with pytest.raises(capi.MavlmError):
            ops.layernorm(x, gamma, beta, 1e-12, DT[mode], out=buf, residual=res)
        torch.cuda.synchronize()
        assert bool((buf == SENTINEL).all())


# ------------------------------------------------------------------------------------------------------------------ backward
_BWD = [pytest.param(d, nv, rows, mode, with_res, id=f"nv{nv}-D{d}-rows{rows}-{mode}-{'res' if with_res else 'nores'}")
        for d, nv in L.BACKWARD_CASES for rows in (5, 300) for mode in ("bf16", "fp16") for with_res in (True, False)]


@pytest.mark.parametrize("d,nv,rows,mode,with_res", _BWD)
def test_layernorm_backward_form_vs_fp64(d, nv, rows, mode, with_res):
    """layernorm_bwd_kernel<T, 2 / 8 / 16>: 512 workgroups of 4 waves over 5 rows (most workgroups hold no row and write a zero
    partial) and over 300.  The gates of test_gpu_backward_m64.py::test_layernorm_bwd_m64_vs_fp64: dz per 64-row block within
    BWD_BLOCK x the floor of float64 dz rounded to the output grid; dgamma and dbeta per 256 columns within F32_SUM_BLOCK x the
    fp32 floor.  Twice, the same bits."""
    assert (d // 4 + 63) // 64 <= nv and (nv == 1 or (d // 4 + 63) // 64 > nv // 2)
    eps = 1e-12
    x = _randn((rows, d), rows + d + 7, 1.5, 0.25)
    res = _randn((rows, d), rows + d + 8).to(DT[mode]) if with_res else None
    dy = _randn((rows, d), rows + d + 9, 0.7).to(DT[mode])
    gamma = (1.0 + 0.2 * _randn((d,), rows + d + 10).to(DT[mode])).float()
    dz, dg, db = ops.layernorm_bwd(dy, x, res, gamma, eps)
    again = ops.layernorm_bwd(dy, x, res, gamma, eps)
    assert torch.equal(again[0], dz) and torch.equal(again[1], dg) and torch.equal(again[2], db)
    z = x.double() + (res.double() if with_res else 0.0)
    mu = z.mean(dim=1, keepdim=True)
    rstd = 1.0 / torch.sqrt((z - mu).square().mean(dim=1, keepdim=True) + eps)
    xh = (z - mu) * rstd
    g = dy.double() * gamma.double()
    dz64 = rstd * (g - g.mean(dim=1, keepdim=True) - xh * (g * xh).mean(dim=1, keepdim=True))
    z32 = x + (res.float() if with_res else 0.0)                 # plain torch fp32 of the same sums (the fp32 floor)
    mu32 = z32.mean(dim=1, keepdim=True)
    xh32 = (z32 - mu32) * torch.rsqrt((z32 - mu32).square().mean(dim=1, keepdim=True) + eps)
    gates = [floor_gate("dz", dz, dz64, 64, d, mode, BWD_BLOCK),
             f32_sum_gate("dgamma", dg, (dy.double() * xh).sum(dim=0), (dy.float() * xh32).sum(dim=0), 256),
             f32_sum_gate("dbeta", db, dy.double().sum(dim=0), dy.float().sum(dim=0), 256)]
    print(f"\n[layernorm bwd NV={nv} D={d} rows={rows} {mode} residual={with_res}]\n  " + "\n  ".join(str(g) for g in gates))
    assert all(g.ok for g in gates), [str(g) for g in gates if not g.ok]


def test_layernorm_backward_refuses_more_than_4096_columns():
    d, rows = L.BACKWARD_REFUSED, 5
    x, dy = _randn((rows, d), 71), _randn((rows, d), 72).bfloat16()
    with pytest.raises(capi.MavlmError):
        ops.layernorm_bwd(dy, x, None, torch.ones(d, device="cuda"), 1e-12)
    torch.cuda.synchronize()
