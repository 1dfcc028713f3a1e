"""CPU: the table of tests/mass_cases.py - the launches of tests/test_gpu_probability_mass.py - against the plans of the C library
(no kernel is launched), under the hooks the GPU test sets, and what the table covers: every plane count class, a workgroup range
over several units, units cut inside their query tiles, the ragged edges on both axes."""
import ctypes

import pytest

import memory_augmented_vlm_amd  # noqa: F401
from memory_augmented_vlm_amd import _capi as capi
import mass_cases as T


@pytest.fixture
def lib(request):
    lib = capi.lib()
    request.addfinalizer(lambda: (lib.mavlm_set_attention_colsum_wgs(0), lib.mavlm_set_attention_streamk_min_tiles(64),
                                  lib.mavlm_set_attention_streamk_waves(0), lib.mavlm_set_attention_impl(0)))
    return lib


def _plan(lib, R, S, H, wgs=0):
    info = (ctypes.c_int32 * 2)()
    capi.check(lib.mavlm_set_attention_colsum_wgs(wgs), "colsum wgs")
    capi.check(lib.mavlm_attention_colsum_plan(R, S, H, info), "colsum plan")
    return info[0], info[1]


def _planes_of(segs):
    """most workgroups over one unit"""
    per = {}
    for g, u, _, _ in segs:
        per.setdefault(u, set()).add(g)
    return max(len(v) for v in per.values())


def test_column_sum_cases_are_what_the_library_plans(lib):
    for R, S, H, wgs, G, planes in T.COLSUM_CASES:
        assert _plan(lib, R, S, H, wgs) == (G, planes), (R, S, H, wgs)
        segs = T.colsum_segments(R, S, H, G)
        ntq, units = -(-R // 64), -(-S // 128) * H
        # the mirror of the kernel's arithmetic: every (unit, tile) exactly once, and the library's plane count
        assert sorted((u, t) for _, u, t0, n in segs for t in range(t0, t0 + n)) == [(u, t) for u in range(units) for t in range(ntq)]
        assert _planes_of(segs) == planes, (R, S, H, wgs)
        assert lib.mavlm_attention_colsum_floats(R, S, H) >= planes * H * S
        assert bool(T.colsum_seam_tiles(R, S, H, G)) == (planes > 1)
    for (R, S, H), plan in T.BATCH_PLANS.items():
        assert _plan(lib, R, S, H) == plan
    assert {(R, S, H) for hw, _, H, R, S in T.BATCH_CASES if hw == 128} == set(T.BATCH_PLANS)
    assert max(p for _, p in T.BATCH_PLANS.values()) > 1
    R, H, keys, plans = T.VARLEN_CASE
    assert [_plan(lib, R, s, H) for s in keys] == plans
    assert len({g for g, _ in plans}) == len(plans) and min(p for _, p in plans) == 1 and max(p for _, p in plans) > 1
    assert min(keys) < 128
    # the register-staged kernel (impl 2) writes one plane whatever the shape
    capi.check(lib.mavlm_set_attention_impl(2), "impl")
    assert all(_plan(lib, R, S, H, wgs)[1] == 1 for R, S, H, wgs, _, _ in T.COLSUM_CASES)


def test_column_sum_cases_cover_the_seams_and_the_edges():
    cases = T.COLSUM_CASES
    planes = [c[5] for c in cases]
    assert 1 in planes and 2 in planes and max(planes) >= 3
    spans, cuts = False, False
    for R, S, H, _, G, _ in cases:
        per = {}
        for g, u, tq0, nt in T.colsum_segments(R, S, H, G):
            per.setdefault(g, []).append(u)
            cuts |= tq0 > 0                       # a workgroup that starts inside a unit: the tiles before belong to another
        spans |= any(len(v) >= 2 for v in per.values())
    assert spans and cuts
    assert {0, 1, 63} <= {c[0] % 64 for c in cases} and min(c[0] for c in cases) < 32
    assert {0, 4, 127} <= {c[1] % 128 for c in cases} and min(c[1] for c in cases) < 32
    assert any(c[2] & (c[2] - 1) for c in cases)
    assert {w for _, _, _, w, _, _ in cases} == {0, 64, 200, 1024}
    assert all(R % 32 for _, R, _, _ in T.WIDE_CASES) and {hd for hd, _, _, _ in T.WIDE_CASES} == {128, 448}
    assert {(hd, qg, kg) for hd, _, _, _, qg, kg in T.MAP_CASES} >= {(hd, qg, kg) for hd in (128, 448) for qg, kg in ((1, 4), (7, 196), (64, 4))}
    assert all(R % qg or qg == 1 for _, R, _, _, qg, _ in T.MAP_CASES) and all(S % kg for _, _, S, _, _, kg in T.MAP_CASES)


def test_frame_score_forms_are_what_the_library_plans(lib):
    """the forward's plan under the hooks of every form: the plain grid, and stream-K plans of 4- and 8-wave workgroups with at
    least one cut unit (fewer than a whole round), at every key count of the table"""
    info = (ctypes.c_int32 * 4)()
    R, H = T.FRAMES_R, T.FRAMES_H
    for name, min_tiles, waves, _, want in T.FRAMES_FORMS:
        capi.check(lib.mavlm_set_attention_streamk_min_tiles(min_tiles), "min tiles")
        capi.check(lib.mavlm_set_attention_streamk_waves(waves), "waves")
        for P, F in T.FRAMES_PF:
            capi.check(lib.mavlm_attention_plan(R, P * F, H, info), "plan")
            assert list(info) == want, (name, P, F, list(info))
            assert lib.mavlm_attention_frames_ws_floats(R, P * F, H, P) > 0
            if want[1]:
                cut = 0
                while lib.mavlm_attention_plan_unit(R, P * F, H, 0, 0, cut) >= 0:
                    cut += 1
                assert 0 < cut == -(-R // (32 * want[0])) * H - want[1], (name, cut)
    assert R % 128 and R % 256 and {P % 64 == 0 for P, _ in T.FRAMES_PF} == {True, False}
    assert all(F <= 32 for _, F in T.FRAMES_PF)                 # the form with its entries in LDS (FR = 3) takes at most 32 frames
