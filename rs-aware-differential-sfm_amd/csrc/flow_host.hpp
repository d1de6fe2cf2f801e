// flow_host.hpp -- what the clip ABI (flow_seq_host.hip) takes from the DeepFlow host driver (flow_host.hip): the argument check, the
// workspace and the one level loop that serves single pairs and clips alike.
#pragma once

#include <stdint.h>

#include <vector>

#include "../../include/rsdsfm_flow.h"
#include "flow_kernels.hpp"
#include "rsdsfm_internal.hpp"

namespace rsdsfm {
namespace flowhost {

constexpr int kLaneTables = 16;  // the most lanes rsdsfm_set_sequence_lanes admits

// resize tables of one axis (tests/flow_spec_numpy.py resize_table): offsets into the workspace's int / float tables
struct AxisTab {
    size_t i0, i1, w0, w1;
};

// A pyramid workspace for batches of up to B pairs: one device allocation with the resize tables, B + 1 frame pyramids and B pairs'
// working planes, rebuilt when the size, the pyramid or B changes.  A context owns two (flow_ws; alternating calls rebuild neither):
// the pair one (B = 1, the single-pair kernels of flow_kernels.hip) and the clip one (B from rsdsfm_set_flow_batch, the batched
// kernels of flow_seq_kernels.hip at every B).  The ring of B fields of rsdsfm_solve_video_dev is a second allocation of the clip
// one, made on first use; so are the lanes' scratch pose tables of rsdsfm_rectify_video_dev.
struct FlowWs {
    const bool pair;  // which kernel set and error prefix: never n == 1 (a clip at B = 1 runs the batched kernels)
    int B = 0, rows = 0, cols = 0, min_size = -1;
    double downscale = 0.0, sigma = -1.0;
    void* d_buf = nullptr;
    void* d_ring = nullptr;
    size_t ring_stride = 0;  // bytes between the ring's fields
    double* d_tables = nullptr;  // kLaneTables x rows x 12 doubles: per lane R (rows x 9) then t (rows x 3)
    std::vector<int> lr, lc;
    std::vector<size_t> lvl_off;  // pyramid level offsets (floats) into each frame's pyramid
    std::vector<AxisTab> down_x, down_y, up_x, up_y;  // [l]: level l -> l + 1 / level l + 1 -> l
    int radius = 0;
    std::vector<int32_t> ti;
    std::vector<float> tf;  // taps first, then the resize weights
    size_t stride = 0, pstride = 0;  // floats from one pair's plane to the next / from one frame's pyramid to the next
    int32_t* d_ti = nullptr;
    float* d_tf = nullptr;
    float* pyr = nullptr;   // B + 1 pyramids
    float* set[2][6] = {};  // per level parity: u, v, du0, dv0, du1, dv1 (B planes each)
    float* avg = nullptr;
    float* d[FLOW_NDERIV] = {};
    float* c[FLOW_NCOEF] = {};  // one block: the pre-smoothing's horizontal pass of the B + 1 frames uses it first
    explicit FlowWs(bool is_pair) : pair(is_pair) {}
};

// sides in [2, 16384], channels 1 or 3, parameters valid (NULL = the defaults); *p receives the parameters to use
int check_args(Ctx* c, int rows, int cols, int channels, const rsdsfm_flow_params* pp, rsdsfm_flow_params* p);
// the context's pair (Ctx::flow_pair) or clip (Ctx::flow_clip) workspace, made on first use; flow_release frees both
FlowWs* flow_ws(Ctx* c, bool pair);
int ensure_flow_ws(Ctx* c, FlowWs* w, int B, int rows, int cols, const rsdsfm_flow_params& p);
// one batch on an ensured workspace: device frames[0 .. n] -> device flows[0 .. n - 1], n <= w->B; every launch serves all n pairs
int flow_enqueue(Ctx* c, const FlowWs* w, const uint8_t* const* frames, int n, int channels, const rsdsfm_flow_params& p, double* const* flows);
// the host-pointer calls, on an ensured workspace: per batch of up to w->B pairs upload n + 1 frames, flow_enqueue, download n fields,
// synchronise
int flow_staged(Ctx* c, const FlowWs* w, const uint8_t* const* frames, int nframes, int channels, const rsdsfm_flow_params& p, double* const* flows);

}  // namespace flowhost
}  // namespace rsdsfm
