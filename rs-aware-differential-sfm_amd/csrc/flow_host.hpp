// flow_host.hpp -- host helpers of the DeepFlow front end shared by the single-pair driver (flow_host.hip) and the sequence driver
// (flow_seq_host.hip): argument checks, the defaults, the pyramid geometry, the Gaussian taps and the resize tables.
#pragma once

#include <stdint.h>

#include <vector>

#include "../../include/rsdsfm_flow.h"
#include "rsdsfm_internal.hpp"

namespace rsdsfm {
namespace flowhost {

constexpr int kFlowMaxSide = 16384;

bool params_ok(const rsdsfm_flow_params& p);
rsdsfm_flow_params defaults();
void levels_of(int rows, int cols, const rsdsfm_flow_params& p, std::vector<int>& lr, std::vector<int>& lc);
std::vector<float> gauss_taps(double sigma);

// resize tables of one axis (tests/flow_spec_numpy.py resize_table): offsets into the workspace's int / float tables
struct AxisTab {
    size_t i0, i1, w0, w1;
};
AxisTab axis_table(int src, int dst, std::vector<int32_t>& ti, std::vector<float>& tf);

// sides in [2, 16384], channels 1 or 3, parameters valid (NULL = the defaults); *p receives the parameters to use
int check_args(Ctx* c, int rows, int cols, int channels, const rsdsfm_flow_params* pp, rsdsfm_flow_params* p);

}  // namespace flowhost
}  // namespace rsdsfm
