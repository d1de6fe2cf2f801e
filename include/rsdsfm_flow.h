/*
 * rsdsfm_flow.h -- C ABI of the dense optical-flow front end (DeepFlow's variational part) on the MI355X.
 *
 * Replaces Camera::calculateDeepFlow of the reference (camera.cc:253-277): two 8-bit frames -> gray -> OpenCV-style DeepFlow
 * (cv::optflow::createOptFlow_DeepFlow, OpenCV 3.4) -> a dense flow field rows x cols x 2 doubles, row-major, (u, v) per pixel
 * (cv::Mat_<cv::Point_<double>>, camera.cc:274) -- the layout rsdsfm_solve_frame_dev reads.  The algorithm is defined by
 * tests/flow_spec_numpy.py (float32, one rounding per operation) and reproduced bit for bit; DESIGN.md section 12 describes it.
 * Parity with OpenCV's own DeepFlow is not pinned (OpenCV is not a dependency).
 *
 * Images: rows x cols x channels bytes, row-major; channels 3 = BGR (converted with OpenCV's integer COLOR_BGR2GRAY), 1 = gray.
 */
#ifndef RSDSFM_FLOW_H
#define RSDSFM_FLOW_H

#include "rsdsfm.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Parameters and defaults of cv::optflow::createOptFlow_DeepFlow (OpenCV 3.4; camera.cc:258 uses the defaults).
 * Valid: sigma in [0, 16], min_size >= 0, downscale in (0, 1), both iteration counts > 0, alpha > 0, delta >= 0, gamma >= 0,
 * omega in (0, 2); every value finite. */
typedef struct rsdsfm_flow_params {
    double sigma;                    /* pre-smoothing Gaussian (0.6) */
    int32_t min_size;                /* the pyramid stops before a level with a side <= min_size (25) or < 2 */
    double downscale;                /* pyramid factor per level (0.95) */
    int32_t fixed_point_iterations;  /* outer iterations per level (5) */
    int32_t sor_iterations;          /* red-black SOR iterations per outer iteration (25) */
    double alpha;                    /* smoothness weight (1; the refinement runs with 4 x alpha) */
    double delta;                    /* brightness-constancy weight (0.5; runs with delta / 3) */
    double gamma;                    /* gradient-constancy weight (5; runs with gamma / 3) */
    double omega;                    /* SOR relaxation (1.6) */
} rsdsfm_flow_params;

/* camera.cc:258 (createOptFlow_DeepFlow()): fills *out with the defaults above.  Host only. */
int rsdsfm_flow_default_params(rsdsfm_flow_params* out);

/* camera.cc:253-277, the pyramid DeepFlow builds: level 0 = rows x cols, next side = (int)(side * downscale + 0.5), stop before a level
 * with a side <= min_size or below 2 (the floor of the frame itself, whatever min_size: a 1 x 1 level has no neighbour to smooth
 * against), or one that would not shrink.  Host only, no GPU needed.  *n: on entry the capacity of level_rows /
 * level_cols (which may be NULL to ask for the count), on return the number of levels; RSDSFM_ERR_INVALID when the capacity is
 * too small (*n then holds the count needed) or the arguments are bad. */
int rsdsfm_flow_levels(int32_t rows, int32_t cols, const rsdsfm_flow_params* params_or_null, int32_t* n, int32_t* level_rows,
                       int32_t* level_cols);

/* camera.cc:253-277 on device buffers: d_img1 / d_img2 rows x cols x channels bytes, d_flow rows x cols x 2 doubles.  Enqueued on
 * the context's stream; returns without waiting (rsdsfm_solve_frame_dev can follow on the same buffer).  params NULL = defaults.
 * rows, cols in [2, 16384]; channels 1 or 3.  The pyramid workspace (about 210 bytes per pixel) belongs to the context and is
 * allocated on first use and whenever the size or the pyramid changes. */
int rsdsfm_deep_flow_dev(rsdsfm_ctx* ctx, const uint8_t* d_img1, const uint8_t* d_img2, int32_t rows, int32_t cols, int32_t channels,
                         const rsdsfm_flow_params* params_or_null, double* d_flow);

/* camera.cc:253-277 on host buffers (same layouts); synchronous. */
int rsdsfm_deep_flow(rsdsfm_ctx* ctx, const uint8_t* img1, const uint8_t* img2, int32_t rows, int32_t cols, int32_t channels,
                     const rsdsfm_flow_params* params_or_null, double* flow);

#ifdef __cplusplus
}
#endif

#endif /* RSDSFM_FLOW_H */
