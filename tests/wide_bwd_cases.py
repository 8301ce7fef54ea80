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
# 64 wide would be one output row a step and four ring segments: refused by the plan, (wide, general, general)
REFUSED_64 = wd(2, 128, 128, 2, 64)
