"""Wide module layers (wide_cases.py) trained under CIMQ_OPT_WIDE_BWD on the channel-chunked compact-state backward:
the case table shared by test_wide_bwd_host.py and test_gpu_wide_bwd.py.  Plain data built with rect_cases.case."""
from wide_cases import wd

WIDE_BWD = ("wide", "wide_bwd", "wide_bwd")

# B1 .. B5, B7 (B6 is B1 and B2 with an all-equal alpha_cim: the literal flag at w3a3 and at w4a4)
CASES = [
    wd(2, 128, 128, 16, 16),                   # B1: T = 9, several channel chunks and bands
    wd(2, 256, 128, 4, 16, bits=4),            # B2: w4a4 word pairs, rectangular, two images per grad_w stage
    wd(2, 128, 256, 16, 16, bits=2, xbar=64),  # B3: 16 output blocks, one K-step
    wd(2, 512, 512, 8, 8),                     # B4: T = 36, a tile straddling a chunk edge
    wd(2, 144, 160, 8, 8),                     # B5: 16-row last tile, partial output groups (10 blocks)
    wd(2, 128, 128, 4, 32),                    # B7: 32 wide -- two ring segments a row, the kw fold across them
]
B1, B2, B3, B4, B5, B7 = range(6)
LITERAL = [B1, B2]

# N1 .. N4: batches at which wide_bwd_plan_compute's two batch-dependent launch parameters leave their trivial value
# (every case above runs RB = 1 and nstage = 1).  grad_x's band height: rb = 8, halved while B * ceil(H / rb) < 256.
# grad_w's stages per workgroup: nstage = ceil(stages / min(512 / pairs, gen_chunks, stages)) with stages = B * P / 128
# and pairs = C / 16 * O / 32 (here 8: 64 chunks at the most).  "plan": the (bands, slabs) cimq_module_wide_bwd_plan
# must answer, and with them RB = ceil(H / bands) and nstage = ceil(stages / slabs), both > 1 in every case.
BATCH_CASES = [
    # N1: RB = 8 (two bands, the interior band edge at row 8, three ring steps a band); 256 stages, nstage = 4: a
    # chunk is two whole images
    wd(128, 128, 32, 16, 16, plan=(2, 64)),
    # N2: RB = 4 (four bands, two steps a band); 160 stages, nstage = 3, 54 chunks: every other chunk starts
    # mid-image, the last chunk holds one stage
    wd(80, 128, 32, 16, 16, plan=(4, 54)),
    # N3: RB = 8 on H = 12: bands of 8 and 4 rows with 5 and 3 steps (Wo = 32: two output rows a step, two ring
    # segments a row); 384 stages, nstage = 6: three stages an image
    wd(128, 128, 32, 12, 32, plan=(2, 64)),
    # N4: w4a4 word pairs; RB = 4 (two bands of two steps); 128 stages, nstage = 2
    wd(128, 128, 32, 8, 16, bits=4, plan=(2, 64)),
]
N1, N2, N3, N4 = range(4)


def batch_plan(c, slabs):
    """(stages, nstage) of a case whose plan answers ``slabs`` pixel chunks: 128-pixel grad_w stages in the batch and
    stages per workgroup"""
    stages = c["B"] * c["H"] * c["W"] // 128
    return stages, -(-stages // slabs)


def stage_images(c, nstage, chunk):
    """the images whose pixels chunk ``chunk``'s stages hold (cim_bwd_gw_wide_kernel: stage s of the batch is pixels
    128 s .. 128 s + 127 of [B][P]; a chunk is nstage consecutive stages, the last one whatever is left)"""
    P, stages = c["H"] * c["W"], c["B"] * c["H"] * c["W"] // 128
    lo, hi = chunk * nstage, min(stages, (chunk + 1) * nstage)
    return sorted({m // P for s in range(lo, hi) for m in (128 * s, 128 * s + 127)})


# 64 wide would be one output row a step and four ring segments: refused by the plan, (wide, general, general)
REFUSED_64 = wd(2, 128, 128, 2, 64)
