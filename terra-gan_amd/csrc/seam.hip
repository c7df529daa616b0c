// Seam correction of a filled DSM by a harmonic delta surface (mvp_gan/src/seam_correct.py).
//
//   tg_seam_delta   classifies every pixel and writes the delta raster D that fill_voids then completes: the ring (filled hole
//                   pixels with a known 4-neighbour) gets its target minus the fill, known pixels and unfilled holes get 0
//                   (fixed), the other filled hole pixels get NaN (the unknowns of the harmonic solve)
//   tg_seam_apply   known pixels bit for bit, filled holes fill + delta, unfilled holes NaN
//
// One thread per pixel over the flat index (a wave reads 64 consecutive pixels of a row); only hole pixels read neighbours.
// Determinism: every value is computed by one thread in a fixed order; the counters are integer atomics (sums, and a maximum
// on the bits of a non-negative float).  No kernel uses scratch.
// Inputs near FLT_MAX: if an order-1 target overflows, e - g can be +inf in one direction and -inf in another; d is then NaN, so
// that pixel, still counted as ring, becomes an unknown of the solve.  Terrain heights are nowhere near that.
#include <math.h>

#include "common.h"
#include "raster_known.h"

static inline hipStream_t S(tg_stream_t s) { return (hipStream_t)s; }

__global__ __launch_bounds__(256) void seam_delta_kernel(RasterIn in, const float* __restrict__ filled, int H, int W, int order,
                                                         float* __restrict__ delta, int32_t* __restrict__ counts) {
    __shared__ uint32_t red[4][TG_SEAM_NCOUNTS];
    const int64_t n = (int64_t)H * W;
    uint32_t ring = 0, interior = 0, unfilled = 0, mx = 0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        float z;
        if (rs_known(in, i, z)) {
            delta[i] = 0.f;
            continue;
        }
        const float g = filled[i];
        if (!isfinite(g)) {
            delta[i] = 0.f;
            ++unfilled;
            continue;
        }
        const int y = (int)((uint32_t)i / (uint32_t)W), x = (int)((uint32_t)i - (uint32_t)y * (uint32_t)W);
        float acc = 0.f;
        int cnt = 0;
        // one known neighbour q = p + dir: e = 2 z_q - z_q2 when the second pixel is known too (order 1), else z_q
        auto side = [&](int dy, int dx) {
            const int qy = y + dy, qx = x + dx;
            if (qy < 0 || qy >= H || qx < 0 || qx >= W) return;
            float zq;
            if (!rs_known(in, (int64_t)qy * W + qx, zq)) return;
            float e = zq;
            if (order == 1) {
                const int ry = qy + dy, rx = qx + dx;
                float z2;
                if (ry >= 0 && ry < H && rx >= 0 && rx < W && rs_known(in, (int64_t)ry * W + rx, z2)) e = __fmaf_rn(2.f, zq, -z2);
            }
            acc = __fadd_rn(acc, __fsub_rn(e, g));       // differences first: no cancellation at |z| ~ 1000 m
            ++cnt;
        };
        side(-1, 0);
        side(0, -1);
        side(0, 1);
        side(1, 0);
        if (cnt) {
            const float d = __fdiv_rn(acc, (float)cnt);
            delta[i] = d;
            ++ring;
            const uint32_t b = __float_as_uint(fabsf(d));
            mx = b > mx ? b : mx;
        } else {
            delta[i] = __int_as_float(0x7fc00000);
            ++interior;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        ring += __shfl_xor(ring, o, 64);
        interior += __shfl_xor(interior, o, 64);
        unfilled += __shfl_xor(unfilled, o, 64);
        const uint32_t t = __shfl_xor(mx, o, 64);
        mx = t > mx ? t : mx;
    }
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        red[w][TG_SEAM_RING] = ring;
        red[w][TG_SEAM_INTERIOR] = interior;
        red[w][TG_SEAM_UNFILLED] = unfilled;
        red[w][TG_SEAM_MAX_BITS] = mx;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t r = 0, t = 0, u = 0, m = 0;
        for (int q = 0; q < 4; ++q) {
            r += red[q][TG_SEAM_RING];
            t += red[q][TG_SEAM_INTERIOR];
            u += red[q][TG_SEAM_UNFILLED];
            m = red[q][TG_SEAM_MAX_BITS] > m ? red[q][TG_SEAM_MAX_BITS] : m;
        }
        // integers: the totals do not depend on the order (each is below H * W < 2^31; |d| bits are below 2^31 too)
        if (r) atomicAdd(&counts[TG_SEAM_RING], (int32_t)r);
        if (t) atomicAdd(&counts[TG_SEAM_INTERIOR], (int32_t)t);
        if (u) atomicAdd(&counts[TG_SEAM_UNFILLED], (int32_t)u);
        if (m) atomicMax(&counts[TG_SEAM_MAX_BITS], (int32_t)m);
    }
}

__global__ __launch_bounds__(256) void seam_apply_kernel(RasterIn in, const float* __restrict__ filled,
                                                         const float* __restrict__ delta, int64_t n, float* __restrict__ out) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        float z;
        if (rs_known(in, i, z)) {
            out[i] = z;                                  // known pixels pass through bit for bit
            continue;
        }
        const float g = filled[i];
        out[i] = isfinite(g) ? __fadd_rn(g, delta[i]) : __int_as_float(0x7fc00000);
    }
}

// ---- host side ----------------------------------------------------------------------------------------------------------
static int seam_size_check(const char* who, int H, int W) {
    TG_REQUIRE(H > 0 && W > 0 && (int64_t)H * W < ((int64_t)1 << 31), "%s: raster %dx%d must be non-empty with H*W < 2^31", who,
               H, W);
    return TG_OK;
}

extern "C" int tg_seam_delta(const float* dem, const float* mask, int use_nodata, float nodata, const float* filled, int H, int W,
                             int order, float* delta, int32_t* counts, tg_stream_t stream) {
    if (int rc = seam_size_check("tg_seam_delta", H, W)) return rc;
    TG_REQUIRE(order == 0 || order == 1, "tg_seam_delta: order %d must be 0 or 1", order);
    TG_REQUIRE(dem && filled && delta && counts, "tg_seam_delta: null pointer");
    const hipStream_t s = S(stream);
    if (hipMemsetAsync(counts, 0, TG_SEAM_NCOUNTS * sizeof(int32_t), s) != hipSuccess) {
        tg_set_error("tg_seam_delta: hipMemsetAsync failed");
        return TG_ERR_LAUNCH;
    }
    const RasterIn in{dem, mask, use_nodata, nodata};
    const int64_t n = (int64_t)H * W;
    hipLaunchKernelGGL(seam_delta_kernel, dim3(ew_grid(n, 256)), dim3(256), 0, s, in, filled, H, W, order, delta, counts);
    TG_CHECK_LAUNCH("seam_delta_kernel");
    return TG_OK;
}

extern "C" int tg_seam_apply(const float* dem, const float* mask, int use_nodata, float nodata, const float* filled,
                             const float* delta_filled, int H, int W, float* out, tg_stream_t stream) {
    if (int rc = seam_size_check("tg_seam_apply", H, W)) return rc;
    TG_REQUIRE(dem && filled && delta_filled && out, "tg_seam_apply: null pointer");
    const RasterIn in{dem, mask, use_nodata, nodata};
    const int64_t n = (int64_t)H * W;
    hipLaunchKernelGGL(seam_apply_kernel, dim3(ew_grid(n, 256)), dim3(256), 0, S(stream), in, filled, delta_filled, n, out);
    TG_CHECK_LAUNCH("seam_apply_kernel");
    return TG_OK;
}
