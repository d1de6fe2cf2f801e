// flow_check.hpp -- the forward-backward flow check (include/rsdsfm_flow_check.h): what flow_check_kernels.hip and flow_check_host.hip share.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "flow_kernels.hpp"
#include "rsdsfm_internal.hpp"

namespace rsdsfm {

// The pairs of one launch, a kernel-argument table as flow_enqueue's (pair index = blockIdx.z).  masked, resid and count may be NULL per
// pair; masked[q] may equal fwd[q].
struct FlowCheckPtrs {
    const double* fwd[kFlowSeqMaxPairs];
    const double* bwd[kFlowSeqMaxPairs];
    unsigned char* mask[kFlowSeqMaxPairs];
    double* masked[kFlowSeqMaxPairs];
    double* resid[kFlowSeqMaxPairs];
    long long* count[kFlowSeqMaxPairs];
};

// one launch for npairs <= kFlowSeqMaxPairs pairs of rows x cols fields (sides in [2, 16384], masks 4-byte aligned: checked by the caller);
// the counters must be zero when it runs
hipError_t flow_check_launch(hipStream_t s, const FlowCheckPtrs& t, int npairs, int rows, int cols, double a1, double a2);

void flow_check_release(Ctx* c);  // flow_check_host.hip: the context's checked-flow workspace (Ctx::flow_check)

}  // namespace rsdsfm
