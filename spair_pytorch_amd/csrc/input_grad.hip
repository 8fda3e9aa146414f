// Gradient of the training step with respect to its input image (SpairStepIO.grad_x).  In the reference the image reaches the loss three ways:
// the backbone, the glimpse STN (border padding) and the BCE target.  Two kernels, both plain gathers with a fixed summation order (no
// atomics, so grad_x is bit-for-bit repeatable):
//  * k_glimpse_adjoint: dx_gl[b] = sum over the cells n of sample b of Wy_n^T dG_n Wx_n per channel -- the transpose of the forward glimpse
//    (stn.hip): Wy / Wx are its bilinear row / column weights after the border clip, so samples outside the image pile onto the edge pixels.
//    One workgroup per 16 x 16 pixel tile of one sample; it first marks, in an LDS bit set, the cells whose clipped footprint touches the
//    tile, then every thread walks that set in cell order for its pixel.
//  * k_stem_dgrad: the stem conv's data gradient (a transposed convolution with C = 1..3 outputs) from the gated d act0, cropped to the
//    unpadded image.  Its epilogue is the single writer of grad_x: it adds dx_gl and the BCE-target term g * (log1p(-r) - log(r)), r the
//    recon -- torch's binary_cross_entropy gradient with respect to its target, not clamped: +inf where r == 0, -inf where r == 1.
#include "cells.h"
#include "stn_math.h"

#include <algorithm>

#define IG_TILE 16
#define IG_MAX_CELLS 1025

// the unclipped source coordinate of stn_src_coord_b (same operations, so it agrees with the forward's coordinate inside the image)
__device__ __forceinline__ float ig_raw_coord(float scale, float shift, float base, int nsrc, int ac) {
    const float g = fmaf(scale, base, shift);
    return ac ? (g + 1.f) * 0.5f * (float)(nsrc - 1) : fmaf(g + 1.f, (float)nsrc, -1.f) * 0.5f;
}

// bilinear weight of source index q in output sample j (the forward's taps x0 = floor(coord), x0 + 1 < n, after the border clip)
__device__ __forceinline__ float ig_tap_weight(float scale, float shift, float base, int nsrc, int ac, int q) {
    float cc, m;
    stn_src_coord_b(scale, shift, base, nsrc, ac, true, cc, m);
    const int q0 = (int)floorf(cc);
    const float w1 = cc - (float)q0;
    return (q0 == q ? 1.f - w1 : 0.f) + (q0 + 1 == q ? w1 : 0.f);
}

// samples j in [lo, hi] of one axis that can have a tap on source index q (a superset; the exact weights decide), from the unclipped end
// coordinates.  A non-increasing or non-finite axis: every sample.
__device__ __forceinline__ void ig_sample_range(float u0, float u1, int P, int n, int q, int& lo, int& hi) {
    lo = 0; hi = P - 1;
    const float beta = P > 1 ? (u1 - u0) / (float)(P - 1) : 0.f;
    if (!(beta > 0.f) || !isfinite(u0) || !isfinite(beta)) return;
    if (q > 0) lo = (int)fminf(fmaxf(floorf(((float)q - 1.f - u0) / beta) - 1.f, 0.f), (float)(P - 1));
    if (q < n - 1) hi = (int)fminf(fmaxf(floorf(((float)q + 1.f - u0) / beta) + 1.f, 0.f), (float)(P - 1));
}

// clipped pixel footprint [lo, hi] of one axis of a glimpse (every pixel if the axis is not increasing / not finite)
__device__ __forceinline__ void ig_footprint(float scale, float shift, int P, int n, int ac, int& lo, int& hi) {
    float c0, c1, m;
    stn_src_coord_b(scale, shift, stn_base(0, P, ac), n, ac, true, c0, m);
    stn_src_coord_b(scale, shift, stn_base(P - 1, P, ac), n, ac, true, c1, m);
    lo = 0; hi = n - 1;
    if (!(c1 >= c0) || !isfinite(c0) || !isfinite(c1)) return;
    lo = (int)fmaxf(floorf(c0), 0.f);
    hi = (int)fminf(floorf(c1) + 1.f, (float)(n - 1));
}

// grid (ceil(Iw/16), ceil(I/16), B), 256 threads; row r = k * B + b for cell k of sample b (cells.h); dgl [rows][ld] in (c, i, j) order;
// out [B][C][I][Iw], every element written (x: the Iw columns, y: the I rows)
__global__ __launch_bounds__(256) void k_glimpse_adjoint(const float* __restrict__ nbox, int B, int ncell, const float* __restrict__ dgl, int ld,
                                                         float* __restrict__ out, int C, int I, int Iw, int P, int ac) {
    __shared__ unsigned int hit[(IG_MAX_CELLS + 31) / 32];
    const int b = blockIdx.z;
    const int tx0 = blockIdx.x * IG_TILE, ty0 = blockIdx.y * IG_TILE;
    const int nw = (ncell + 31) / 32;
    for (int i = threadIdx.x; i < nw; i += blockDim.x) hit[i] = 0u;
    __syncthreads();
    for (int k = threadIdx.x; k < ncell; k += blockDim.x) {
        const float4 nb = *reinterpret_cast<const float4*>(nbox + ((size_t)k * B + b) * 4);
        int xlo, xhi, ylo, yhi;
        ig_footprint(nb.z, 2.f * nb.x - 1.f, P, Iw, ac, xlo, xhi);
        ig_footprint(nb.w, 2.f * nb.y - 1.f, P, I, ac, ylo, yhi);
        if (xlo <= tx0 + IG_TILE - 1 && xhi >= tx0 && ylo <= ty0 + IG_TILE - 1 && yhi >= ty0) atomicOr(&hit[k >> 5], 1u << (k & 31));   // OR: order-free
    }
    __syncthreads();
    const int x = tx0 + (threadIdx.x & (IG_TILE - 1)), y = ty0 + (threadIdx.x / IG_TILE);
    if (x >= Iw || y >= I) return;
    const int PP = P * P;
    float acc[3] = {0.f, 0.f, 0.f};
    const float bx0 = stn_base(0, P, ac), bx1 = stn_base(P - 1, P, ac);
    for (int wi = 0; wi < nw; ++wi) {
        unsigned int m = hit[wi];
        while (m) {
            const int k = wi * 32 + __builtin_ctz(m);
            m &= m - 1u;
            const size_t r = (size_t)k * B + b;
            const float4 nb = *reinterpret_cast<const float4*>(nbox + r * 4);
            const float sx = nb.z, hx = 2.f * nb.x - 1.f, sy = nb.w, hy = 2.f * nb.y - 1.f;
            int jlo, jhi, ilo, ihi;
            ig_sample_range(ig_raw_coord(sx, hx, bx0, Iw, ac), ig_raw_coord(sx, hx, bx1, Iw, ac), P, Iw, x, jlo, jhi);
            ig_sample_range(ig_raw_coord(sy, hy, bx0, I, ac), ig_raw_coord(sy, hy, bx1, I, ac), P, I, y, ilo, ihi);
            const float* g = dgl + r * ld;
            for (int i = ilo; i <= ihi; ++i) {
                const float wy = ig_tap_weight(sy, hy, stn_base(i, P, ac), I, ac, y);
                if (wy == 0.f) continue;
                for (int j = jlo; j <= jhi; ++j) {
                    const float wx = ig_tap_weight(sx, hx, stn_base(j, P, ac), Iw, ac, x);
                    if (wx == 0.f) continue;
                    const float w = wy * wx;
                    for (int c = 0; c < C; ++c) acc[c] = fmaf(w, g[c * PP + i * P + j], acc[c]);
                }
            }
        }
    }
    for (int c = 0; c < C; ++c) out[(((size_t)b * C + c) * I + y) * Iw + x] = acc[c];
}

__device__ __forceinline__ void ig_load8(const float* p, float* v) {
    const float4 a = *reinterpret_cast<const float4*>(p), b = *reinterpret_cast<const float4*>(p + 4);
    v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
}
__device__ __forceinline__ void ig_load8(const __bf16* p, float* v) {
    const bf16x8 a = *reinterpret_cast<const bf16x8*>(p);
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = (float)a[e];
}

// 16 lanes per output pixel (b, y, x), lane l takes channels 8l .. 8l+7 (+128 per round) of every tap; the 16 partial sums are reduced in a
// fixed butterfly.  dact: [B][Hout][Wout][Cout] (gated by the stem's ReLU); w: conv_0's [Cout][C][k][k], staged in LDS as [C][k][k][Cout].
// grad_x [B][C][I][Iw] = the data gradient at padded (y + pre, x + pre) + add (nullable) + bce_g * (log1p(-r) - log(r)) with r = clamp(aux.y)
template <class T>
__global__ __launch_bounds__(256) void k_stem_dgrad(const T* __restrict__ dact, const float* __restrict__ w, int B, int C, int I, int Iw, int pre,
                                                    int k, int s, int Hout, int Wout, int Cout, const float* __restrict__ add, const float2* __restrict__ aux,
                                                    const float* __restrict__ bce_g, float* __restrict__ grad_x) {
    extern __shared__ float wsh[];
    const int nwt = Cout * C * k * k;
    for (int i = threadIdx.x; i < nwt; i += blockDim.x) {
        const int co = i / (C * k * k), rem = i - co * C * k * k;       // rem = (ci * k + ky) * k + kx
        wsh[rem * Cout + co] = w[i];
    }
    __syncthreads();
    const long long npx = (long long)B * I * Iw;
    const int lane = threadIdx.x & 15;
    const float g = bce_g ? *bce_g : 0.f;
    // a persistent grid: the weights are staged once per workgroup, not once per 16 pixels.  Whole 16-lane groups take the same trip
    // count, so the butterfly below stays within live lanes
    for (long long p = (long long)blockIdx.x * 16 + (threadIdx.x >> 4); p < npx; p += (long long)gridDim.x * 16) {
        const int b = (int)(p / ((long long)I * Iw)), yx = (int)(p - (long long)b * I * Iw), y = yx / Iw, x = yx - y * Iw;
        const int yp = y + pre, xp = x + pre;
        float acc[3] = {0.f, 0.f, 0.f};
        for (int ky = yp % s; ky < k && ky <= yp; ky += s) {
            const int oy = (yp - ky) / s;
            if (oy >= Hout) continue;
            for (int kx = xp % s; kx < k && kx <= xp; kx += s) {
                const int ox = (xp - kx) / s;
                if (ox >= Wout) continue;
                const T* row = dact + (((size_t)b * Hout + oy) * Wout + ox) * Cout;
                for (int co = lane * 8; co < Cout; co += 128) {
                    float v[8];
                    ig_load8(row + co, v);
                    for (int c = 0; c < C; ++c) {
                        const float* wr = wsh + ((c * k + ky) * k + kx) * Cout + co;
#pragma unroll
                        for (int e = 0; e < 8; ++e) acc[c] = fmaf(wr[e], v[e], acc[c]);
                    }
                }
            }
        }
        for (int c = 0; c < C; ++c) {
#pragma unroll
            for (int o = 8; o >= 1; o >>= 1) acc[c] += __shfl_xor(acc[c], o, 16);
        }
        if (lane != 0) continue;
        for (int c = 0; c < C; ++c) {
            const size_t i = (((size_t)b * C + c) * I + y) * Iw + x;
            float v = acc[c];
            if (add) v += add[i];
            if (bce_g) {
                const float pre_v = aux[i].y;
                const float r = pre_v < 0.f ? 0.f : (pre_v > 1.f ? 1.f : pre_v);      // recon = clamp(pre, 0, 1) (a NaN stays NaN)
                v += g * (log1pf(-r) - logf(r));
            }
            grad_x[i] = v;
        }
    }
}

int input_grad_glimpse(const float* nbox, int B, int ncell, const float* dgl, int ld, float* out, int C, int I, int Iw, int P, int ac, hipStream_t s) {
    if (B <= 0 || ncell <= 0 || ncell > IG_MAX_CELLS || C < 1 || C > 3 || I <= 0 || Iw <= 0 || P <= 0 || ld < C * P * P) return SPAIR_ERR_SHAPE;
    if (!nbox || !dgl || !out) return SPAIR_ERR_SHAPE;
    hipLaunchKernelGGL(k_glimpse_adjoint, dim3((Iw + IG_TILE - 1) / IG_TILE, (I + IG_TILE - 1) / IG_TILE, B), dim3(256), 0, s, nbox, B, ncell, dgl, ld,
                       out, C, I, Iw, P, ac);
    SPAIR_CHECK_LAUNCH();
    return SPAIR_OK;
}

int input_grad_stem(const void* dact, int dact_bf16, const float* w, int B, int C, int I, int Iw, int pre, int k, int s, int Hout, int Wout, int Cout,
                    const float* add, const float* aux, const float* bce_g, float* grad_x, hipStream_t st) {
    if (B <= 0 || C < 1 || C > 3 || I <= 0 || Iw <= 0 || pre < 0 || k < 1 || s < 1 || Hout <= 0 || Wout <= 0 || Cout <= 0 || (Cout & 7))
        return SPAIR_ERR_SHAPE;
    if (!dact || !w || !grad_x || (bce_g && !aux)) return SPAIR_ERR_SHAPE;
    const size_t lds = (size_t)Cout * C * k * k * sizeof(float);
    if (lds > 65536) return SPAIR_ERR_UNSUPPORTED;
    const long long npx = (long long)B * I * Iw;
    const dim3 grid((unsigned)std::min<long long>((npx + 15) / 16, (long long)spair_num_cus() * 8));
    if (dact_bf16)
        hipLaunchKernelGGL(k_stem_dgrad<__bf16>, grid, dim3(256), lds, st, reinterpret_cast<const __bf16*>(dact), w, B, C, I, Iw, pre, k, s,
                           Hout, Wout, Cout, add, reinterpret_cast<const float2*>(aux), bce_g, grad_x);
    else
        hipLaunchKernelGGL(k_stem_dgrad<float>, grid, dim3(256), lds, st, reinterpret_cast<const float*>(dact), w, B, C, I, Iw, pre, k, s,
                           Hout, Wout, Cout, add, reinterpret_cast<const float2*>(aux), bce_g, grad_x);
    SPAIR_CHECK_LAUNCH();
    return SPAIR_OK;
}

// unit entries (include/spair_hip.h)
extern "C" int spair_input_grad_glimpse(const float* nbox, int B, int ncell, const float* dglimpse, int ld_gl, float* out, int C, int I, int P,
                                        int align_corners, void* stream) {
    return input_grad_glimpse(nbox, B, ncell, dglimpse, ld_gl, out, C, I, I, P, align_corners, (hipStream_t)stream);
}
extern "C" int spair_input_grad_stem(const void* dact0, int dact_bf16, const float* w, int B, int C, int I, int pad_pre, int k, int s, int Hout,
                                     int Cout, const float* add, float* grad_x, void* stream) {
    return input_grad_stem(dact0, dact_bf16, w, B, C, I, I, pad_pre, k, s, Hout, Hout, Cout, add, nullptr, nullptr, grad_x, (hipStream_t)stream);
}
