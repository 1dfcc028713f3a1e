"""CPU: the plans that are part of a result's rounding - key splits of small grids, the levelled stream-K schedule, the
rule for computing the frame scores inside the forward - are pure host functions of the shape in the C library, and the
oracle's emulation re-states them (oracle/memory_path.py).  The parity gates rely on the two agreeing for EVERY shape:
swept here without a GPU (no kernel is launched)."""
import ctypes
import itertools

import pytest

import memory_augmented_vlm_amd  # noqa: F401
from memory_augmented_vlm_amd import _capi as capi
from oracle import memory_path as O

ROWS = [1, 100, 128, 784, 1568, 3136, 4100, 8192, 8320, 12544, 25088]
KEYS = [1, 64, 196, 588, 1000, 1024, 4032, 4096, 6272, 12544, 62720, 250880]
HEADS = [1, 2, 3, 8, 64]


@pytest.fixture(scope="module")
def lib():
    return capi.lib()


def test_attention_plans_match_the_oracle(lib):
    info = (ctypes.c_int32 * 4)()
    for R, S, H in itertools.product(ROWS, KEYS, HEADS):
        capi.check(lib.mavlm_attention_plan(R, S, H, info), "plan")
        G, QB, full, levels = O.streamk_plan(R, S, H)
        ns, _ = O.split_plan(R, S, H)
        assert info[1] == G, (R, S, H)
        if G:
            assert info[0] == QB // 32 and info[2] == len(levels) and info[3] == 1, (R, S, H)
        else:
            assert info[3] == ns, (R, S, H)
        # a workspace is needed exactly when a schedule cuts keys
        need = lib.mavlm_attention_ws_floats(R, S, H)
        assert (need > 0) == bool(G or ns > 1), (R, S, H)
        if G:
            assert need == G * len(levels) * (QB * 128 + QB), (R, S, H)


def test_streamk_unit_order_is_a_bijection_and_matches_the_oracle(lib):
    """Round 4: the levelled stream-K schedule deals its units XCD-major (every XCD walks a contiguous range of the head-major
    unit order).  Positions -> units must be a bijection (every unit exactly once, whole or cut), the C map and the oracle's
    must agree, and at the bench launch (2 videos x 8 heads x 49 blocks of 256 queries) an XCD owns exactly two heads."""
    for R, S, H in [(12544, 6272, 16), (12544, 6272, 8), (12544, 12544, 16), (12544, 125440, 8), (1568, 6272, 64), (8320, 4096, 8),
                    (25088, 6272, 8), (100000, 4096, 3), (1100, 6400, 64)]:
        G, QB, full, levels = O.streamk_plan(R, S, H)
        if not G:
            continue
        units = -(-R // QB) * H
        seen = []
        for si in range(full):
            for v in range(G):
                u = lib.mavlm_attention_plan_unit(R, S, H, -1, si, v)
                assert u == O.streamk_unit_of_round(G, full, levels, si, v), (R, S, H, si, v)
                seen.append(u)
        for lv, (k, base, n) in enumerate(levels):
            for ul in range(n):
                u = lib.mavlm_attention_plan_unit(R, S, H, lv, 0, ul)
                assert u == O.streamk_unit_of_level(G, full, levels, lv, ul), (R, S, H, lv, ul)
                seen.append(u)
        assert sorted(seen) == list(range(units)), (R, S, H)
        # the workgroups of one XCD (virtual ids [x G/8, (x+1) G/8)) walk a contiguous unit range
        W = G // 8
        for x in range(8):
            mine = [O.streamk_unit_of_round(G, full, levels, si, v) for si in range(full) for v in range(x * W, (x + 1) * W)]
            for lv, (k, base, n) in enumerate(levels):
                mine += [O.streamk_unit_of_level(G, full, levels, lv, ul) for ul in range(n) if (ul << k) // W == x]
            assert sorted(mine) == list(range(min(mine), max(mine) + 1)), (R, S, H, x)
    G, QB, full, levels = O.streamk_plan(12544, 6272, 16)
    assert (G, QB, full) == (256, 256, 3)
    assert [O.streamk_unit_of_round(G, full, levels, 0, 32 * x) for x in range(8)] == [98 * x for x in range(8)]


def test_wide_head_plans_match_the_oracle(lib):
    """head_dim 448: the levelled stream-K plan of the 32-query-wave kernel (more 128-query units than 256 workgroups; H up to
    the heads of a row batch) and the key splits of the small single-video grids; head_dim 256 (16-query kernel): splits only."""
    info = (ctypes.c_int32 * 4)()
    for R, S, H in itertools.product(ROWS, KEYS, [1, 2, 8, 32, 64]):
        G, full, levels = O.streamk_plan_wide(R, S, H)
        ns, _ = O.split_plan_wide(R, S, H)
        capi.check(lib.mavlm_attention_hd_plan_info(R, S, H, 448, info), "plan info")
        assert info[0] == G, (R, S, H)
        need = lib.mavlm_attention_hd_ws_floats(R, S, H, 448)
        if G:
            assert info[1] == full and info[2] == len(levels) and info[3] == 1, (R, S, H)
            assert need == G * len(levels) * (128 * 448 + 128), (R, S, H)
            cuts = O.streamk_split_tiles_wide(R, S, H)
            assert len(cuts) == sum(n for _, _, n in levels), (R, S, H)
            nt = -(-S // 32)
            for rng in cuts.values():                         # a cut unit's ranges tile its keys exactly, in order
                assert rng[0][0] == 0 and rng[-1][1] == nt and all(a[1] == b[0] for a, b in zip(rng, rng[1:])), (R, S, H)
        else:
            assert info[3] == ns, (R, S, H)
            assert (need > 0) == (ns > 1), (R, S, H)
            if ns > 1:
                assert need == ns * (R * H * 448 + H * R), (R, S, H)
        capi.check(lib.mavlm_attention_hd_plan_info(R, S, H, 256, info), "plan info")
        assert info[0] == 0 and info[3] == ns, (R, S, H)
        assert lib.mavlm_attention_hd_ws_floats(R, S, H, 256) == (ns * (R * H * 256 + H * R) if ns > 1 else 0), (R, S, H)


@pytest.fixture
def level_hooks(lib, monkeypatch, request):
    """set the stream-K hooks of the library and their mirrors in the oracle together; both are restored afterwards"""
    request.addfinalizer(lambda: (lib.mavlm_set_attention_streamk_min_tiles(64), lib.mavlm_set_attention_streamk_waves(0)))

    def set_hooks(min_tiles, waves):
        capi.check(lib.mavlm_set_attention_streamk_min_tiles(min_tiles), "min tiles")
        capi.check(lib.mavlm_set_attention_streamk_waves(waves), "waves")
        monkeypatch.setattr(O, "STREAMK_MIN_TILES", min_tiles)
        monkeypatch.setattr(O, "STREAMK_WAVES", waves)
    return set_hooks


def _narrow_plan_equals(lib, R, S, H, waves, G, full, levels):
    """head_dim 128: C plan and oracle against the literal (G, whole rounds, levels); the unit map is a bijection"""
    info = (ctypes.c_int32 * 4)()
    capi.check(lib.mavlm_attention_plan(R, S, H, info), "plan")
    QB = 32 * waves
    assert list(info) == [waves, G, len(levels), 1], (R, S, H, list(info))
    assert O.streamk_plan(R, S, H) == (G, QB, full, levels), (R, S, H, O.streamk_plan(R, S, H))
    assert lib.mavlm_attention_plan_unit(R, S, H, -1, full - 1, 0) >= 0 and lib.mavlm_attention_plan_unit(R, S, H, -1, full, 0) == -1
    assert lib.mavlm_attention_plan_unit(R, S, H, len(levels), 0, 0) == -1
    seen = [lib.mavlm_attention_plan_unit(R, S, H, -1, si, v) for si in range(full) for v in range(G)]
    for lv, (k, base, n) in enumerate(levels):
        assert lib.mavlm_attention_plan_unit(R, S, H, lv, 0, n) == -1, (R, S, H, lv)
        for ul in range(n):
            u = lib.mavlm_attention_plan_unit(R, S, H, lv, 0, ul)
            assert u == O.streamk_unit_of_level(G, full, levels, lv, ul), (R, S, H, lv, ul)
            seen.append(u)
    assert sorted(seen) == list(range(-(-R // QB) * H)), (R, S, H)
    assert lib.mavlm_attention_ws_floats(R, S, H) == G * len(levels) * (QB * 128 + QB), (R, S, H)


def _wide_plan_equals(lib, R, S, H, G, full, levels):
    info = (ctypes.c_int32 * 4)()
    capi.check(lib.mavlm_attention_hd_plan_info(R, S, H, 448, info), "plan info")
    assert list(info) == [G, full, len(levels), 1], (R, S, H, list(info))
    assert O.streamk_plan_wide(R, S, H) == (G, full, levels), (R, S, H, O.streamk_plan_wide(R, S, H))
    cuts = O.streamk_split_tiles_wide(R, S, H)
    nqb = -(-R // 128)
    # position order: the whole rounds take the first full * G units, the levels the rest, each unit once
    assert sorted(h * nqb + b for h, b in cuts) == list(range(full * G, nqb * H)), (R, S, H)
    assert lib.mavlm_attention_hd_ws_floats(R, S, H, 448) == G * len(levels) * (128 * 448 + 128), (R, S, H)


def test_streamk_level_cases_are_what_the_library_plans(lib, level_hooks):
    """The table of tests/streamk_cases.py - the plans the GPU tests of the cut levels launch - against the C library and the
    oracle under the same hooks: G, whole rounds, the level list, the unit bijection; and the table's coverage: every cut width the
    plan rule can produce, a plan of at least four levels and one with two or more whole rounds per kernel."""
    import streamk_cases as T
    for kernel, R, S, H, G, full, levels in T.STREAMK_CASES:
        level_hooks(T.MIN_TILES, T.WAVES[kernel])
        if kernel == "wide":
            _wide_plan_equals(lib, R, S, H, G, full, levels)
        else:
            _narrow_plan_equals(lib, R, S, H, T.WAVES[kernel], G, full, levels)
    level_hooks(T.MIN_TILES, 0)
    for kernel, nb, R, S, H, G, full, levels in T.BATCH_CASES:
        nqb = -(-R // (128 if kernel == "wide" else 256))
        if kernel == "wide":
            _wide_plan_equals(lib, R, S, H, G, full, levels)
            cut = {h * nqb + b for h, b in O.streamk_split_tiles_wide(R, S, H)}
            assert lib.mavlm_attention_batch_ws_floats(R, S, H, nb, 448) == lib.mavlm_attention_hd_ws_floats(R, S, H, 448)
        else:
            _narrow_plan_equals(lib, R, S, H, 8, G, full, levels)
            cut = {lib.mavlm_attention_plan_unit(R, S, H, lv, 0, ul) for lv, (_, _, n) in enumerate(levels) for ul in range(n)}
            assert lib.mavlm_attention_batch_ws_floats(R, S, H, nb, 128) == lib.mavlm_attention_ws_floats(R, S, H)
        videos = {u // nqb // (H // nb) for u in cut}
        # the XCD-affine order of head_dim 128 deals cut units to every video; the position order of the wide kernel cuts the
        # tail of the head-major order, which reaches back over a video boundary only from three videos on
        assert videos == (set(range(nb)) if kernel != "wide" else ({1} if nb == 2 else {1, 2})), (kernel, nb, videos)
    for kernel, want in (("w8", {1, 2, 3, 4, 5}), ("w4", {2, 3, 4, 5}), ("wide", {1, 2, 3, 4, 5})):
        mine = T.cases_of(kernel)
        assert {k for c in mine for k, _, _ in c[6]} == want, kernel
        assert max(len(c[6]) for c in mine) >= 4 and max(c[5] for c in mine) >= 2, kernel
        assert any(c[1] % (32 * (T.WAVES[kernel] or 4)) and len(c[6]) > 1 for c in mine), kernel       # ragged and multi-level
        assert any(-(-c[2] // (32 if kernel == "wide" else 64)) < 32 and c[6][-1][0] == 5 for c in mine), kernel   # empty pieces


def test_split_kv_cases_cover_every_plane_count(lib):
    """The split-KV shapes of tests/streamk_cases.py under the default hooks: the C plans and the oracle give the listed plane
    counts, which cover 2 .. 8 at head_dim 128 and 2 .. 7 (the most the wide plan gives over a sweep) at 448, each at least once
    with a ragged last key tile and a short last plane."""
    import streamk_cases as T
    info = (ctypes.c_int32 * 4)()
    ragged = {128: set(), 448: set()}
    for R, S, H, n128, n448 in T.SPLIT_CASES:
        if n128 is not None:
            capi.check(lib.mavlm_attention_plan(R, S, H, info), "plan")
            ns, tps = O.split_plan(R, S, H)
            assert info[1] == 0 and info[3] == n128 == ns, (R, S, H, list(info), ns)
            if S % 64 and -(-S // 64) % tps:
                ragged[128].add(ns)
        if n448 is not None:
            capi.check(lib.mavlm_attention_hd_plan_info(R, S, H, 448, info), "plan info")
            ns, tps = O.split_plan_wide(R, S, H)
            assert info[0] == 0 and info[3] == n448 == ns, (R, S, H, list(info), ns)
            if S % 32 and -(-S // 32) % tps:
                ragged[448].add(ns)
    assert ragged[128] == set(range(2, 9)) and ragged[448] == set(range(2, 8)), ragged
    assert max(O.split_plan_wide(R, S, H)[0] for R, S, H in itertools.product(ROWS, KEYS, [1, 2, 3, 8, 32])) == 7


def test_frame_score_rule_matches_the_oracle(lib):
    for R, H, P in itertools.product(ROWS, HEADS, [4, 60, 64, 100, 196, 198]):
        for F in (1, 2, 3, 32, 40, 64, 65):
            S = F * P
            assert bool(lib.mavlm_frame_scores_fused(R, S, H, P)) == O.frame_scores_fused(R, S, H, P), (R, S, H, P)
            assert (lib.mavlm_attention_frames_ws_floats(R, S, H, P) > 0) == (P % 4 == 0 and P >= 64 and F <= 64), (R, S, H, P)
        assert not lib.mavlm_frame_scores_fused(R, 3 * P + 4, H, P)          # keys that are not whole frames
    try:
        capi.check(lib.mavlm_set_frame_score_mode(0), "mode")
        assert not lib.mavlm_frame_scores_fused(12544, 6272, 8, 196)
    finally:
        lib.mavlm_set_frame_score_mode(1)
    assert lib.mavlm_frame_scores_fused(12544, 6272, 8, 196) and not lib.mavlm_frame_scores_fused(1568, 6272, 8, 196)


def test_column_sum_plan_is_consistent(lib):
    info = (ctypes.c_int32 * 2)()
    for R, S, H in itertools.product(ROWS, KEYS, [1, 3, 8]):
        capi.check(lib.mavlm_attention_colsum_plan(R, S, H, info), "colsum plan")
        wgs, planes = info[0], info[1]
        nkb, ntq = -(-S // 128), -(-R // 64)
        total = nkb * H * ntq
        assert 1 <= wgs <= min(512, total) and planes >= 1, (R, S, H)
        assert lib.mavlm_attention_colsum_floats(R, S, H) >= planes * H * S, (R, S, H)
        # the planes bound: a unit's ntq tiles are spread over at most ceil((ntq - 1) / floor(total / wgs)) + 1 workgroups
        q = total // wgs
        assert planes <= (ntq - 1 + q - 1) // q + 1, (R, S, H)
