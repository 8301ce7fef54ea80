// cimq_part_v7.hip -- the v7 backward's launch sequence (cimq_v7_launch.h) instantiated for w2a2, w3a3 and w8a8
// layers (w4a4: cimq_part_v7_44.hip).  Own translation unit of libcimq.so.
#include "cimq_v7_launch.h"

namespace cimq {

template CIMQ_V7_SIG(2, 2);
template CIMQ_V7_SIG(3, 3);
template CIMQ_V7_SIG(8, 8);

}  // namespace cimq
