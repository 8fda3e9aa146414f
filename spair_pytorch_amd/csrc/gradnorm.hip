// Global L2 norm of the flat gradient buffer, per parameter segment and in total, and the fused Adam step that clips by it
// (include/spair_hip.h, "gradient norm and clipping"; torch.nn.utils.clip_grad_norm_ + torch.optim.Adam).  A streaming reduction: 16-byte
// aligned loads, float64 squares and sums, partials stored per work item and summed in a fixed order -- no atomics, so the norm, the
// scale and through them the parameters are bit-identical from run to run.
#include <cmath>
#include "common.h"
#include "spair_hip.h"

static_assert(SPAIR_GRAD_CHUNK % 1024 == 0, "one trip of k_grad_sumsq's body is 256 lanes x 4 floats");

// ---- per work item: sum of squares of grads[lo, hi) ---------------------------------------------------------------------------------
// One workgroup per item.  Only the 4-byte alignment of the buffer is assumed: the elements in front of the first 16-byte boundary
// (head, < 4) and behind the last whole float4 (tail, < 4) are read one by one, so that nothing outside [lo, hi) is read at all.
// Order: a lane adds its head element, then its float4s v = lane, lane + 256, .. (x, y, z, w), then its tail element; the 64 lanes of a
// wave through a butterfly; the four waves in order through LDS.
__global__ __launch_bounds__(256) void k_grad_sumsq(const float* __restrict__ g, const long long* __restrict__ items,
                                                    double* __restrict__ partial) {
    __shared__ double s_wave[4];
    const long long lo = items[3 * (long long)blockIdx.x + 1], hi = items[3 * (long long)blockIdx.x + 2];
    const int t = threadIdx.x;
    const long long len = hi > lo ? hi - lo : 0;
    long long head = (long long)(((16u - (unsigned)(reinterpret_cast<unsigned long long>(g + lo) & 15u)) & 15u) >> 2);
    if (head > len) head = len;
    const float4* __restrict__ body = reinterpret_cast<const float4*>(g + lo + head);
    const long long nvec = (len - head) >> 2;
    const long long tail_lo = lo + head + 4 * nvec;
    const long long tail = lo + len - tail_lo;
    double acc = 0.0;
    if (t < head) {
        const double d = (double)g[lo + t];
        acc += d * d;
    }
    for (long long v0 = t; v0 < nvec; v0 += 1024) {
        float4 x[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const long long v = v0 + 256 * k;
            x[k] = v < nvec ? body[v] : make_float4(0.f, 0.f, 0.f, 0.f);
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const double a = (double)x[k].x, b = (double)x[k].y, c = (double)x[k].z, d = (double)x[k].w;
            acc += a * a;
            acc += b * b;
            acc += c * c;
            acc += d * d;
        }
    }
    if (t < tail) {
        const double d = (double)g[tail_lo + t];
        acc += d * d;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off, 64);
    if ((t & 63) == 0) s_wave[t >> 6] = acc;
    __syncthreads();
    if (t == 0) partial[blockIdx.x] = ((s_wave[0] + s_wave[1]) + s_wave[2]) + s_wave[3];
}

// ---- one workgroup: items -> segments -> total -> {norm, scale}, counters ----------------------------------------------------------
#define GN_TILE 1024
__global__ __launch_bounds__(256) void k_grad_norm_finish(const long long* __restrict__ items, long long n_items, int nseg,
                                                          const double* __restrict__ partial, double* __restrict__ seg_sumsq,
                                                          float* __restrict__ out, float max_norm, float norm_eps, int* __restrict__ clip) {
    __shared__ double s_seg[SPAIR_GRAD_MAX_SEGMENTS];
    __shared__ double s_tile[GN_TILE];
    __shared__ int s_first[SPAIR_GRAD_MAX_SEGMENTS + 1];      // first item of each segment (items are sorted by segment)
    const int t = threadIdx.x;
    for (int s = t; s <= nseg; s += 256) s_first[s] = (int)n_items;
    for (int s = t; s < nseg; s += 256) s_seg[s] = 0.0;
    __syncthreads();
    for (long long i = t; i < n_items; i += 256) {
        const long long seg = items[3 * i];
        if (seg >= 0 && seg < nseg && (i == 0 || items[3 * (i - 1)] != seg)) s_first[seg] = (int)i;
    }
    __syncthreads();
    for (long long base = 0; base < n_items; base += GN_TILE) {
        const int cnt = (int)(n_items - base < GN_TILE ? n_items - base : GN_TILE);
        for (int i = t; i < cnt; i += 256) s_tile[i] = partial[base + i];
        __syncthreads();
        for (int s = t; s < nseg; s += 256) {
            const long long a = s_first[s] > base ? s_first[s] : base;
            const long long b = s_first[s + 1] < base + cnt ? s_first[s + 1] : base + cnt;
            if (a < b) {
                double acc = s_seg[s];
                for (long long i = a; i < b; ++i) acc += s_tile[i - base];
                s_seg[s] = acc;
            }
        }
        __syncthreads();
    }
    for (int s = t; s < nseg; s += 256) seg_sumsq[s] = s_seg[s];
    if (t == 0) {
        double total = 0.0;
        for (int s = 0; s < nseg; ++s) total += s_seg[s];
        const float norm = (float)sqrt(total);
        const bool finite = fabsf(norm) <= 3.402823466e38f;
        float scale = 1.0f;
        if (finite && max_norm > 0.f) scale = fminf(1.0f, max_norm / (norm + norm_eps));
        out[0] = norm;
        out[1] = scale;
        if (scale < 1.0f) clip[0] += 1;
        if (!finite) clip[1] += 1;
    }
}

// ---- k_adam_guarded (misc.hip) on gradients scaled by the device scalar norm_out[1] --------------------------------------------------
__global__ __launch_bounds__(256) void k_adam_clipped(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                      float* __restrict__ v, long long n, float lr, float b1, float b2, float eps,
                                                      float bc1, float sqrt_bc2, const int* __restrict__ skip, int* __restrict__ counters,
                                                      const float* __restrict__ norm_out) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (skip && *skip) {
        if (i == 0) counters[0] += 1;
        return;
    }
    const float norm = norm_out[0], scale = norm_out[1];
    if (!(fabsf(norm) <= 3.402823466e38f)) return;                          // non-finite norm: k_grad_norm_finish counted the step
    if (i >= n) return;
    const float gi = g[i] * scale;
    if (!(fabsf(gi) <= 3.402823466e38f)) { counters[1] = 1; return; }      // NaN or inf
    const float mi = b1 * m[i] + (1.f - b1) * gi;
    const float vi = b2 * v[i] + (1.f - b2) * gi * gi;
    m[i] = mi;
    v[i] = vi;
    const float denom = sqrtf(vi) / sqrt_bc2 + eps;
    p[i] -= (lr / bc1) * (mi / denom);
}

// ---- C ABI (include/spair_hip.h) ---------------------------------------------------------------------------------------------------
extern "C" int spair_grad_chunk(void) { return SPAIR_GRAD_CHUNK; }

extern "C" long long spair_grad_norm_items(const int64_t* seg_lo, const int64_t* seg_hi, int nseg, int64_t n, int64_t* items) {
    if (n <= 0 || nseg < 1 || nseg > SPAIR_GRAD_MAX_SEGMENTS || !seg_lo || !seg_hi) return SPAIR_ERR_SHAPE;
    int64_t end = 0;
    for (int s = 0; s < nseg; ++s) {
        if (seg_lo[s] < end || seg_hi[s] <= seg_lo[s] || seg_hi[s] > n) return SPAIR_ERR_SHAPE;
        end = seg_hi[s];
    }
    long long k = 0;
    for (int s = 0; s < nseg; ++s)
        for (int64_t lo = seg_lo[s]; lo < seg_hi[s]; lo += SPAIR_GRAD_CHUNK, ++k)
            if (items) {
                items[3 * k] = s;
                items[3 * k + 1] = lo;
                items[3 * k + 2] = seg_hi[s] - lo < SPAIR_GRAD_CHUNK ? seg_hi[s] : lo + SPAIR_GRAD_CHUNK;
            }
    return k;
}

extern "C" int spair_grad_norm(const float* grads, const int64_t* items_dev, long long n_items, int nseg, double* partial,
                               double* seg_sumsq, float* out, float max_norm, float norm_eps, int* clip, void* stream) {
    if (!grads || !items_dev || !partial || !seg_sumsq || !out || !clip) return SPAIR_ERR_SHAPE;
    if (nseg < 1 || nseg > SPAIR_GRAD_MAX_SEGMENTS || n_items < nseg || n_items >= (1ll << 31)) return SPAIR_ERR_SHAPE;
    if (!(norm_eps >= 0.f) || std::isnan(max_norm)) return SPAIR_ERR_SHAPE;
    const long long* items = reinterpret_cast<const long long*>(items_dev);
    hipLaunchKernelGGL(k_grad_sumsq, dim3((unsigned)n_items), dim3(256), 0, (hipStream_t)stream, grads, items, partial);
    SPAIR_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_grad_norm_finish, dim3(1), dim3(256), 0, (hipStream_t)stream, items, n_items, nseg, partial, seg_sumsq, out,
                       max_norm, norm_eps, clip);
    SPAIR_CHECK_LAUNCH();
    return SPAIR_OK;
}

extern "C" int spair_adam_clipped(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t n, float lr, float beta1,
                                  float beta2, float eps, int step, const int* skip, int* counters, const float* norm_out, void* stream) {
    if (n <= 0 || step < 1 || !params || !grads || !exp_avg || !exp_avg_sq || !counters || !norm_out) return SPAIR_ERR_SHAPE;
    const float bc1 = 1.f - powf(beta1, (float)step);
    const float sqrt_bc2 = sqrtf(1.f - powf(beta2, (float)step));
    hipLaunchKernelGGL(k_adam_clipped, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, params, grads, exp_avg,
                       exp_avg_sq, (long long)n, lr, beta1, beta2, eps, bc1, sqrt_bc2, skip, counters, norm_out);
    SPAIR_CHECK_LAUNCH();
    return SPAIR_OK;
}
