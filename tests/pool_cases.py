"""Wide module layers whose forward kernel stores the 2 x 2 / stride-2 max pool of its epilogue's values
(cimq_module_forward_pool): the case table shared by the host test (test_pool_host.py) and the GPU test
(test_gpu_pool.py).  Plain data built with wide_cases.wd; no fixtures, no device work.

In cim_fwd_wide_kernel a lane holds four pixels of one output row of a 64-pixel m-tile; the row below is Wo pixels on:
the neighbouring 16 lanes at Wo = 4, the other half of the wave at Wo = 8, the next wave at Wo = 16, two waves on at
Wo = 32.  The cases hold every one of those distances, every compile-time slice form (CST 0 / 2 / 3 / 4), both K-step
counts, partial output groups, the literal ADC path, a strided layer and a grid-stride over several images."""
from wide_cases import vgg7_wide, wd

#                                                        Wo   why
CASES = [
    wd(2, 128, 64, 16, 16),                            # P1  16   the next wave; CST 3, two K-steps
    wd(2, 128, 16, 32, 32, xbar=64),                   # P2  32   two waves away; one output block, one K-step
    wd(2, 144, 48, 8, 8),                              # P3   8   in the wave (lane ^ 32); three output blocks
    wd(2, 272, 32, 16, 4, bits=2),                     # P4   4   lane ^ 16, a 16 x 4 image; CST 2.  272 channels: the
                                                       #          smallest multiple of 16 that leaves the whole-C plan here
    wd(2, 128, 80, 16, 16, bits=4),                    # P5  16   CST 4; two output groups (64 + 16)
    wd(2, 128, 32, 16, 16, wb=4, ab=4, wbs=2, abs=2),  # P6  16   4 / 4 bits in 2-bit slices: CST 0, run-time counts
    wd(2, 128, 32, 16, 16, adc=4),                     # P7  16   a multi-bit ADC: the literal path
    wd(2, 128, 32, 32, 32, s=2),                       # P8  16   stride 2: a pooled 8 x 8 plane from a 32 x 32 image
    wd(3, 128, 32, 8, 32),                             # P9  32   four m-tiles an image, odd batch, grid-stride across images
]
P1, P2, P3, P4, P5, P6, P7, P8, P9 = range(9)

# (K-steps, compile-time slice count) of the kernel instance each case runs: all of 2 / 3 / 4 / 0 and both K-step counts
FORMS = [(2, 3), (1, 3), (2, 3), (2, 2), (2, 4), (2, 0), (2, 3), (2, 3), (2, 3)]


def vgg7_pooled(B):
    """the three layers of VGG7 in front of a max-pool: 128 -> 128 @32, 256 -> 256 @16, 512 -> 512 @8"""
    v = vgg7_wide(B)
    return [v[0], v[2], v[4]]


# ---- not poolable ----
WIDE64 = wd(2, 128, 16, 2, 64)        # a wide layer 64 columns wide: the rows of a window are in different m-tiles
OFF_WIDE = [
    wd(2, 16, 16, 8, 32, route=("fwd5", "gx5", "gw5")),
    wd(2, 128, 128, 8, 8, route=("v3", "general", "general")),   # 128 channels at 8 x 8 still fit the whole-C patch
    wd(2, 64, 64, 32, 32, route=("general", "general", "general")),
    wd(128, 64, 64, 1, 1, k=1, p=0, xbar=64, route=("dense", "dense", "dense")),
]
