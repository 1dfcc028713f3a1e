"""The launches of tests/test_gpu_probability_mass.py as literals, shared with the CPU test that pins them to the C library without a
GPU (tests/test_mass_cases_cpu.py).  A change of a plan rule breaks the literals there first, so the coverage of the seams of the
column-sum pass's balanced schedule cannot rot silently.

Column sums (attn_colsum3_kernel): a unit is (128-key block, head) x all 64-query tiles; G workgroups share the flattened (unit,
tile) space evenly; the pieces of a unit go to separate planes.  `colsum_segments` re-states that arithmetic (it is what places
the planted rows either side of every seam); the CPU test holds it to the library through the plane count."""

# (R, S, H, `mavlm_set_attention_colsum_wgs`, G, planes)
COLSUM_CASES = [
    (20, 20, 3, 0, 3, 1),              # R < 32, S < 32, three heads: one ragged tile and one ragged key block per unit
    (200, 260, 2, 0, 6, 1),            # the small shape of test_gpu_colsum_batch.py: S % 128 = 4, one workgroup per unit
    (512, 784, 2, 0, 14, 1),           # R % 64 = 0: the last shape without a cut unit ...
    (513, 784, 2, 0, 15, 2),           # ... MULTI_PLANE, R % 64 = 1: workgroups of 8 tiles over units of 9
    (513, 784, 2, 64, 15, 2),          # (the hook does not move a plan that short ranges cap)
    (1087, 260, 3, 0, 19, 3),          # R % 64 = 63, three planes
    (1215, 255, 3, 0, 14, 4),          # S % 128 = 127, four planes
    (8320, 1024, 8, 0, 512, 9),        # R % 64 = 0, S % 128 = 0: every setting of the hook gives another plan
    (8320, 1024, 8, 64, 64, 1),        # one workgroup per unit again
    (8320, 1024, 8, 200, 200, 5),
    (8320, 1024, 8, 1024, 1024, 17),
]

# row batches: (head width, videos, heads per video, R per video, S) - every video runs the single-video plan of (R, S, H)
BATCH_CASES = [(128, 3, 2, 200, 260), (448, 3, 2, 100, 150), (128, 3, 2, 513, 784)]
BATCH_PLANS = {(200, 260, 2): (6, 1), (513, 784, 2): (15, 2)}

# variable-length row batch: R per video, heads, key counts, and the (G, planes) of every video's own plan
VARLEN_CASE = (513, 2, [784, 260, 20], [(15, 2), (6, 1), (2, 1)])

# wide column sums (attn_colsum_hd_kernel, 32-row tiles, one workgroup per (128-key block, head)): (head_dim, R, S, H)
WIDE_CASES = [(448, 100, 150, 2), (128, 200, 260, 3), (448, 33, 300, 3)]

# fused frame scores (attn_fwd3_kernel FR = 1 / 3): R x H is the smallest grid of 8 heads with cut units that is ragged against
# both unit heights; (P, F): frame boundaries at tile ends (64) and inside tiles and pieces
FRAMES_R, FRAMES_H = 8317, 8
FRAMES_PF = [(64, 4), (68, 4), (100, 3), (196, 3)]
# (name, streamk_min_tiles, streamk_waves, frame_entries_lds, [waves, workgroups, levels, key planes] of mavlm_attention_plan)
FRAMES_FORMS = [("grid", 64, 0, 1, [4, 0, 0, 1]), ("sk4", 1, 4, 1, [4, 512, 1, 1]), ("sk8-scratch", 1, 8, 0, [8, 256, 1, 1]),
                ("sk8-lds", 1, 8, 1, [8, 256, 1, 1])]

# attention maps (attn_group_mass_rows_kernel): (head_dim, R, S, H, q_group, k_group); R = 200 is ragged against q_group 7 and
# 64 and against the 128 rows of a workgroup, S = 590 against both key groups and the 32-key tiles
MAP_CASES = [(hd, 200, 590, H, qg, kg) for hd, H in ((128, 3), (448, 2)) for qg, kg in ((1, 4), (7, 196), (64, 4), (64, 196))]


def colsum_segments(R, S, H, G):
    """[(workgroup, unit, first tile, tiles)] of the balanced schedule, in workgroup order (attn_colsum3_kernel's arithmetic)"""
    ntq = -(-R // 64)
    ttot = -(-S // 128) * H * ntq
    q, rem = divmod(ttot, G)
    segs = []
    for g in range(G):
        b0 = g * q + min(g, rem)
        b1 = b0 + q + (1 if g < rem else 0)
        while b0 < b1:
            u, tq0 = divmod(b0, ntq)
            nt = min(ntq - tq0, b1 - b0)
            segs.append((g, u, tq0, nt))
            b0 += nt
    return segs


def colsum_seam_tiles(R, S, H, G):
    """the query tiles at which some unit is cut between two workgroups (a seam lies before tile t), sorted"""
    return sorted({tq0 for _, _, tq0, _ in colsum_segments(R, S, H, G) if tq0})


def case_id(c):
    return "-".join(str(x) for x in c[:4])
