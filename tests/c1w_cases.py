"""The w8a8 first conv with 32 .. 512 output channels trained under CIMQ_OPT_WIDE_BWD on cim_bwd_c1w_kernel: the case
table shared by test_c1w_host.py and test_gpu_c1w.py.  Plain data built with rect_cases.case."""
from rect_cases import case

C1W = ("v3", "c1w", "c1w")
GENERAL = ("v3", "general", "general")


def routes(c):
    """with the bit; the forward keeps its kernel, the general one where 256 % O != 0 (cim_fwd_v3_kernel's gate)"""
    return (C1W[0] if 256 % c["O"] == 0 else "general",) + C1W[1:]


CASES = [
    case(2, 3, 32, 8, 32, bits=8, signed=1),   # two blocks in one group, two steps, two ring segments a row
    case(2, 3, 32, 16, 8, bits=8),             # W = 8: one step of 16 rows
    case(2, 3, 48, 16, 16, bits=8),            # odd block count: the wcy K-steps straddle two weight slices
    case(3, 3, 128, 16, 16, bits=8),           # two groups of four blocks, the group-partial fold, odd batch
    case(2, 1, 32, 16, 16, bits=8),            # K = 9: one (c, kh) block
    case(2, 3, 32, 16, 8, bits=8, adc=4),      # a multi-bit ADC: the literal path
    case(2, 3, 80, 16, 8, bits=8, signed=1),   # five blocks: a last group of one
    # the widths and step counts c1_fill accepts beyond those above (W <= 32, at most two steps)
    case(2, 3, 32, 32, 32, bits=8, signed=1),  # VGG-small's image: eight steps, the ring reused four times
    case(2, 3, 32, 4, 64, bits=8),             # W = 64: R = 2, four ring segments a row, two steps
    case(2, 3, 32, 8, 64, bits=8, signed=1),   # W = 64, four steps
]
GROUPS = 3    # the case that must report >= 2 groups
LITERAL = 0   # ... that also runs with an all-equal alpha_cim (the literal flag)

# what the bit must not move: 16 channels stay on c1; 2-bit slices, stride 2 and C = 16 (K = 144) on what they had
UNMOVED = [
    case(2, 3, 16, 8, 32, bits=8, signed=1, route=("v3", "c1", "c1")),
    case(2, 3, 32, 16, 16, bits=8, wbs=2, abs=2, route=None),
    case(2, 3, 32, 16, 16, bits=8, s=2, route=None),
    case(2, 16, 32, 16, 16, bits=8, route=None),
]
