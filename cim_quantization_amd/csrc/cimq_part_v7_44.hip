// cimq_part_v7_44.hip -- the v7 backward's launch sequence (cimq_v7_launch.h) instantiated for w4a4 layers in
// 1-bit slices: 16 slice pairs in 8-byte state words (V7W_32X2).  Own translation unit of libcimq.so.
#include "cimq_v7_launch.h"

namespace cimq {

template CIMQ_V7_SIG(4, 4);

}  // namespace cimq
