// stabilize_map_body.hpp -- the STATEMENTS of the stabiliser's map kernel (stage B with the virtual pose; tests/stabilize_spec_numpy.py::forward_map),
// included into the body of stabilize_map_kernel (stabilize_kernels.hip, RSDSFM_STABILIZE_MAP_VISIBLE 0: token for token the code it always
// was) and of stabilize_visible_map_kernel (stabilize_visible_kernels.hip, RSDSFM_STABILIZE_MAP_VISIBLE 1), which also writes the depth in the
// virtual camera, zv, and splats it into the z-buffer (include/rsdsfm_stabilize_visible.h; tests/stabilize_visible_spec_numpy.py::forward_map_depth).
// Shared as text, not as a device function: with the pose handed to an inlined function (by value or by reference) its 12 doubles are loaded
// at the call, not where they are used, and the existing kernel then spills 10 SGPRs (96 -> 106, measured with hipcc -S) -- its code and its
// time would not be the parent's.  The including kernel declares, under these names: depth_cm, lv1, h1, w1, R, t, fx, fy, cx, cy, fyp, rows,
// cols, mode, vp, disp, filled_cm and, VISIBLE, zv (float*) and zbuf (unsigned*).
// RSDSFM_STABILIZE_MAP_VISIBLE 2 (stabilize_search_map_kernel, stabilize_search_kernels.hip; include/rsdsfm_stabilize_search.h): the splat goes
// into kbuf (unsigned long long*) instead of zbuf, as the 64-bit key bits(zv) << 32 | (y cols + x) -- the nearest depth and, on equal depth,
// the smallest source index.  With 0 and 1 the preprocessed text is what it was, token for token.
//
// A 64 x 16 tile of the column-major depth map staged through LDS, the last push step fused, a wave per scanline segment with the scanline's
// pose on the scalar path, the optional filled-depth write-back.  VISIBLE: zv[y cols + x] = (float)pv[2] where that is a positive finite depth,
// else 0 -- 4 B per pixel, coalesced, D's index -- and zbuf[iy cols + ix] = min(., bits(zv)) at the cell the projection's doubles land in: an
// integer atomic minimum without a returned value, skipped when a plain load finds the cell at or below the lane's value already (the cell
// only ever decreases, so a stale value only costs an atomic; the minimum commutes: exact and independent of scheduling).
    constexpr int RPW = kTY / (kCB / kTX);  // scanlines per wave
    __shared__ double s_z[kTX][kTY + 1];
    const int x0 = blockIdx.x * kTX, y0 = blockIdx.y * kTY;
    const int tid = threadIdx.x;
    const int lx = tid & (kTX - 1);
    const int x = x0 + lx;
    const int wv = __builtin_amdgcn_readfirstlane(tid / kTX);
    const int sy = tid & (kTY - 1);  // the staging layout: lanes along y
    double zst[kTX * kTY / kCB];
#pragma unroll
    for (int j = 0; j < kTX * kTY / kCB; ++j) {
        const int xx = x0 + tid / kTY + j * (kCB / kTY), yy = y0 + sy;
        zst[j] = (xx < cols && yy < rows) ? depth_cm[(int64_t)xx * rows + yy] : 0.0;
    }
    double R0[9], t0[3];
#pragma unroll
    for (int i = 0; i < 9; ++i) R0[i] = R[i];
#pragma unroll
    for (int i = 0; i < 3; ++i) t0[i] = t[i];
#pragma unroll
    for (int j = 0; j < kTX * kTY / kCB; ++j) s_z[tid / kTY + j * (kCB / kTY)][sy] = zst[j];
    __syncthreads();
#pragma unroll
    for (int j = 0; j < RPW; ++j) {
        const int ly = wv + j * (kCB / kTX);
        const int y = y0 + ly;  // wave-uniform
        double Rr[9], tr[3];
        const int ys = (mode == 0 && y < rows) ? y : 0;
#pragma unroll
        for (int i = 0; i < 9; ++i) Rr[i] = R[(int64_t)ys * 9 + i];
#pragma unroll
        for (int i = 0; i < 3; ++i) tr[i] = t[(int64_t)ys * 3 + i];
        if (y < rows && x < cols) {
            double z = s_z[lx][ly];
            if (inverse_depth(z) == 0.0) {  // the last push step: level 0 from level 1
                const double rho = push_from(lv1, h1, w1, x, y);
                z = rho > 0.0 ? 1.0 / rho : 0.0;
                s_z[lx][ly] = z;  // (read and written by this thread only)
            }
            double pg[3], pv[3], gx, gy;
            rs_to_gs_point(x, y, z, Rr, tr, R0, t0, fx, fy, cx, cy, pg);
#pragma unroll
            for (int i = 0; i < 3; ++i) pv[i] = ((vp.M[3 * i] * pg[0] + vp.M[3 * i + 1] * pg[1]) + vp.M[3 * i + 2] * pg[2]) + vp.m[i];
            rs_to_gs_project(pv, fx, cx, cy, fyp, gx, gy);
            disp[(int64_t)y * cols + x] = make_float2((float)(gx - (double)x), (float)(gy - (double)y));
#if RSDSFM_STABILIZE_MAP_VISIBLE
            {
                const float zf = (float)pv[2];
                const float zd = (pv[2] > 0.0 && pv[2] < INFINITY && zf < INFINITY) ? zf : 0.0f;  // false for NaN
                zv[(int64_t)y * cols + x] = zd;
                if (zd > 0.0f && gx >= -0.5 && gx < (double)cols - 0.5 && gy >= -0.5 && gy < (double)rows - 0.5) {  // false for NaN
                    const int ix = min((int)(gx + 0.5), cols - 1), iy = min((int)(gy + 0.5), rows - 1);        // gx + 0.5 >= 0: inside the plane
#if RSDSFM_STABILIZE_MAP_VISIBLE == 2
                    unsigned long long* cell = kbuf + ((int64_t)iy * cols + ix);
                    const unsigned long long bits = ((unsigned long long)__float_as_uint(zd) << 32) | (unsigned)(y * cols + x);  // rows cols <= 2^28
#else
                    unsigned* cell = zbuf + ((int64_t)iy * cols + ix);
                    const unsigned bits = __float_as_uint(zd);
#endif
                    if (*cell > bits) atomicMin(cell, bits);
                }
            }
#endif
        }
    }
    if (filled_cm) {  // (uniform)
        __syncthreads();
#pragma unroll
        for (int j = 0; j < kTX * kTY / kCB; ++j) {
            const int sx = tid / kTY + j * (kCB / kTY);
            const int xx = x0 + sx, yy = y0 + sy;
            if (xx < cols && yy < rows) filled_cm[(int64_t)xx * rows + yy] = s_z[sx][sy];
        }
    }
