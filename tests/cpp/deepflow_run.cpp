// deepflow_run.cpp -- Camera::calculateDeepFlow (camera.cc:253-277) through the drop-in C++ mirror (host/camera.h): two frames given to
// addFrameReal, then the flow from frame 1 to frame 2.  Reads two raw BGR images (rows x cols x 3 bytes), writes the flow as raw
// doubles (rows x cols x 2); driven by tests/test_cpp_deepflow.py.
#include <cstdio>
#include <cstdlib>
#include <stdexcept>
#include <vector>

#include "../../rs-aware-differential-sfm_amd/host/camera.h"

static bool read_bgr(const char* path, rsdsfm::ImageBGR& img) {
    FILE* f = std::fopen(path, "rb");
    if (!f) return false;
    const size_t n = (size_t)img.rows() * (size_t)img.cols() * 3;
    const bool ok = std::fread(img.data(), 1, n, f) == n;
    std::fclose(f);
    return ok;
}

int main(int argc, char** argv) {
    if (argc < 6) {
        std::fprintf(stderr, "usage: deepflow_run frame1.bgr frame2.bgr rows cols flow.bin\n");
        return 2;
    }
    const int rows = std::atoi(argv[3]), cols = std::atoi(argv[4]);
    rsdsfm::ImageBGR a(rows, cols), b(rows, cols);
    if (!read_bgr(argv[1], a) || !read_bgr(argv[2], b)) return 3;
    try {
        Camera camera;
        camera.setIntrinsics("galaxy");
        camera.addFrameReal(a);
        camera.addFrameReal(b);
        const rsdsfm::FlowImage flow = camera.calculateDeepFlow(1, 2);
        FILE* f = std::fopen(argv[5], "wb");
        const size_t n = (size_t)rows * (size_t)cols * 2;
        if (!f || std::fwrite(flow.data(), sizeof(double), n, f) != n) return 4;
        std::fclose(f);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    std::printf("ok\n");
    return 0;
}
