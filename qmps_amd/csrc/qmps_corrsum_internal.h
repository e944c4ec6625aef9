// qmps_corrsum_internal.h - what the dispatch of the correlator sums (qmps_corrsum.hip) calls in the kernel files; `Src` is
// OneSiteSource (qmps_corrsum_one_site.h) or TwoSiteSource (qmps_corrsum_two_site.h), both instantiated where the kernels are.
// Arguments are checked by the caller.  Library-internal.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "qmps_kernels.h"

namespace qmps {

struct OneSiteSource;
struct TwoSiteSource;

// D = 2, 4 (qmps_corrsum_small.hip): one kernel per n_ops
template <class Src>
void launch_small(int D, const CorrSumArgs& a, int64_t items, hipStream_t st);
// D = 8, 16 (qmps_corrsum_block.hip); D = 16 takes a.work and a.n_slabs
template <class Src>
void launch_block(int D, const CorrSumArgs& a, int64_t items, hipStream_t st);

}  // namespace qmps
