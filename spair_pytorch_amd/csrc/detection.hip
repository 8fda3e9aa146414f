// Detection metrics on the device: predicted boxes with scores, ranked and matched greedily one-to-one against the true boxes of each image
// at every IoU threshold, then the precision / recall curve pooled over all images and the area under its envelope (average precision).
// Definitions in include/spair_hip.h, "detection metrics".
//
//   k_det_match: one workgroup of 256 per image.  Boxes go to LDS; the keys of the live predictions (order-preserving score bits : ~n)
//                are compacted, padded with zeros to a power of two and ranked by a bitonic sort in LDS, and the boxes are laid out again
//                in ranked order.  The walk over the ranked list is sequential, with the truths over the lanes of a group and one
//                threshold per group: 16-lane groups where K <= 16 (sixteen thresholds in one pass of the workgroup), else 32-lane
//                groups (eight per pass).  A lane keeps its truth box in registers and computes its IoU with four ranked predictions at a
//                time (independent divisions, ahead of the dependent chain); the best free truth is a 16-lane DPP max (for 32 lanes two
//                readlanes more), a ballot of the lanes equal to the max and its lowest set bit: the lowest j on a tie without a second
//                compare.  The taken truths are one 32-bit mask per group.  Per-image integer sums go to the counter block with integer
//                atomics.  (A first version sorted all N keys padded to a power of two, walked with 32-lane groups only -- two passes
//                for the nine default thresholds -- and read key, then box, then computed one IoU per step: 21.5 us with no live
//                prediction and 186 us with all 256 live at B = 256, N = 256, K = 11; profiles/f16_detection.txt has both.)
//   k_det_ap:    one workgroup of 1024 per threshold over the score-sorted tp words, from the last valid record to the first in chunks of
//                4096 (four consecutive records per thread, loaded one chunk ahead): an integer suffix count of the threshold's bit gives TP_i (the total is in
//                the counter block), a running-max scan of TP_i / (i + 1) gives the envelope, and every thread sums the envelope at its
//                own true positives; the 1024 partial sums are added in a fixed tree.  No atomics: bit-identical from run to run.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "common.h"

namespace {

constexpr int DET_MAX_N = 1024;
constexpr int DET_MAX_K = 32;                     // SC_MAXOBJ of scenes.hip
constexpr int DET_MAX_T = 16;
constexpr int DET_THREADS = 256;
constexpr int DET_AP_THREADS = 1024;
constexpr int DET_AP_WAVES = DET_AP_THREADS / 64;
constexpr int DET_AP_PER = 4;
constexpr int DET_AP_CHUNK = DET_AP_THREADS * DET_AP_PER;

typedef unsigned long long u64;

__device__ __forceinline__ bool det_finite(float v) { return fabsf(v) < __builtin_inff(); }       // false for NaN and +-inf

// IoU of corner boxes a and b as the header defines it: every operation rounded once, nothing contracted into an fma
__device__ __forceinline__ float det_iou(float ax0, float ay0, float ax1, float ay1, float bx0, float by0, float bx1, float by1) {
#pragma clang fp contract(off)
    const bool ok = det_finite(ax0) && det_finite(ay0) && det_finite(ax1) && det_finite(ay1) && det_finite(bx0) && det_finite(by0) &&
                    det_finite(bx1) && det_finite(by1);
    const float iw = fmaxf(fminf(ax1, bx1) - fmaxf(ax0, bx0), 0.f);
    const float ih = fmaxf(fminf(ay1, by1) - fmaxf(ay0, by0), 0.f);
    const float inter = iw * ih;
    const float ua = (ax1 - ax0) * (ay1 - ay0);
    const float ub = (bx1 - bx0) * (by1 - by0);
    const float un = (ua + ub) - inter;
    const float q = inter / un;
    return ok && un > 0.f && q > 0.f ? q : 0.f;   // (a NaN un or q compares false; an empty intersection gives +0, never -0)
}

__device__ __forceinline__ float det_add(float a, float b) {
#pragma clang fp contract(off)
    return a + b;
}

__device__ __forceinline__ unsigned det_ordered(float s) {       // unsigned order = float order (s is no NaN; -0 was made +0)
    const unsigned u = __float_as_uint(s);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

template <int CTRL>
__device__ __forceinline__ float dpp_max_(float v) {
    return fmaxf(v, __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xf, 0xf, true)));
}
// Max over each group of GW = 16 or 32 consecutive lanes, result in every lane of the group (v is no NaN).  Four DPP steps give every
// 16-lane row its max; a 32-lane group joins its two rows through scalar registers.
template <int GW>
__device__ __forceinline__ float group_max(float v, int lane) {
    v = dpp_max_<0xB1>(v);      // quad_perm [1,0,3,2]
    v = dpp_max_<0x4E>(v);      // quad_perm [2,3,0,1]
    v = dpp_max_<0x141>(v);     // row_half_mirror
    v = dpp_max_<0x140>(v);     // row_mirror
    if (GW == 16) return v;
    const int i = __builtin_bit_cast(int, v);
    const float lo = fmaxf(__builtin_bit_cast(float, __builtin_amdgcn_readlane(i, 0)), __builtin_bit_cast(float, __builtin_amdgcn_readlane(i, 16)));
    const float hi = fmaxf(__builtin_bit_cast(float, __builtin_amdgcn_readlane(i, 32)), __builtin_bit_cast(float, __builtin_amdgcn_readlane(i, 48)));
    return lane < 32 ? lo : hi;
}

constexpr int DET_UNROLL = 4;                     // ranked predictions whose IoUs a lane computes together (independent divisions)

// GW: lanes per threshold group -- 16 where K <= 16 (sixteen thresholds per pass of the workgroup), else 32 (eight per pass)
template <int GW>
__global__ __launch_bounds__(DET_THREADS) void k_det_match(const float* __restrict__ boxes, const float* __restrict__ scores,
                                                           const float* __restrict__ bbox, const int* __restrict__ count,
                                                           const float* __restrict__ thr, int N, int K, int T, float min_score, int max_det,
                                                           float* __restrict__ score_out, int* __restrict__ tp_out,
                                                           int* __restrict__ order_out, int* __restrict__ n_pred_out,
                                                           int* __restrict__ n_truth_out, u64* __restrict__ counters, float* __restrict__ iou) {
    __shared__ u64 s_key[DET_MAX_N];
    __shared__ float4 s_box[DET_MAX_N];                                  // by prediction index n
    __shared__ float4 s_rbox[DET_MAX_N + DET_UNROLL];                    // by rank r (the walk reads it linearly, a few slots ahead)
    __shared__ int s_tp[DET_MAX_N];
    __shared__ int s_cnt[DET_MAX_T];
    __shared__ int s_n;
    const int tid = threadIdx.x, lane = tid & 63;
    const int b = blockIdx.x;
    const float* sc = scores + (size_t)b * N;
    const float* bx = boxes + (size_t)b * N * 4;
    const float* tb = bbox + (size_t)b * K * 4;

    // what the walk needs from memory, asked for before anything waits: truth j on lane j of every group of GW lanes, threshold
    // pass * G + g on group g
    constexpr int G = DET_THREADS / GW;
    const int g = tid / GW, j = tid % GW;
    const int cnt = min(max(count[b], 0), K);
    float tx0 = 0.f, ty0 = 0.f, tw = 0.f, th_ = 0.f;
    if (j < K) { tx0 = tb[4 * j]; ty0 = tb[4 * j + 1]; tw = tb[4 * j + 2]; th_ = tb[4 * j + 3]; }
    const float thr0 = g < T ? thr[g] : __builtin_nanf("");              // no IoU is >= NaN: an idle group matches nothing
    if (tid == 0) s_n = 0;
    if (tid < DET_MAX_T) s_cnt[tid] = 0;
    for (int r = tid; r < max_det; r += DET_THREADS) s_tp[r] = 0;
    __syncthreads();
    // the live predictions' keys, compacted in any order (the keys are distinct and the sort follows)
    for (int n = tid; n < N; n += DET_THREADS) {
        float s = sc[n];
        s_box[n] = make_float4(bx[4 * n], bx[4 * n + 1], bx[4 * n + 2], bx[4 * n + 3]);
        if (s == s && s >= min_score) {
            if (s == 0.f) s = 0.f;                                       // -0 ranks as +0
            s_key[atomicAdd(&s_n, 1)] = ((u64)det_ordered(s) << 32) | (u64)(~(unsigned)n);
        }
    }
    __syncthreads();
    const int n_pred = s_n;
    const int kept = min(n_pred, max_det);
    const int P2 = n_pred <= 1 ? 1 : 1 << (32 - __clz(n_pred - 1));      // the sort's size: n_pred padded to a power of two with keys 0
    for (int i = n_pred + tid; i < P2; i += DET_THREADS) s_key[i] = 0;
    __syncthreads();

    // rank: bitonic sort of the keys, descending (live keys are above 0: they come first, in ranked order)
    for (int k = 2; k <= P2; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < P2; i += DET_THREADS) {
                const int x = i ^ j;
                if (x > i) {
                    const u64 a = s_key[i], c = s_key[x];
                    if ((i & k) == 0 ? a < c : a > c) { s_key[i] = c; s_key[x] = a; }
                }
            }
            __syncthreads();
        }
    }
    for (int r = tid; r < kept; r += DET_THREADS) s_rbox[r] = s_box[~(unsigned)s_key[r]];
    __syncthreads();

    if (iou) {                                                           // the whole [N][K] matrix, truth slots past cnt included
        float* out = iou + (size_t)b * N * K;
        for (int e = tid; e < N * K; e += DET_THREADS) {
            const int n = e / K, j = e - n * K;
            const float4 p = s_box[n];
            const float x = tb[4 * j], y = tb[4 * j + 1];
            out[e] = det_iou(p.x, p.y, p.z, p.w, x, y, det_add(x, tb[4 * j + 2]), det_add(y, tb[4 * j + 3]));
        }
    }

    // the walk
    const int shift = lane & (64 - GW);                                  // where the group's lanes sit in a ballot
    const float tx1 = det_add(tx0, tw), ty1 = det_add(ty0, th_);
    const bool real = j < cnt;
    for (int pass = 0; pass * G < T; ++pass) {
        const int t = pass * G + g;
        const bool active = t < T;
        const float th = pass == 0 ? thr0 : active ? thr[t] : __builtin_nanf("");
        unsigned taken = 0;
        int ntp = 0;
        for (int r0 = 0; r0 < kept; r0 += DET_UNROLL) {
            float q[DET_UNROLL];
#pragma unroll
            for (int u = 0; u < DET_UNROLL; ++u) {                       // (slots at and past kept hold anything: their IoU is not used)
                const float4 p = s_rbox[r0 + u];
                q[u] = det_iou(p.x, p.y, p.z, p.w, tx0, ty0, tx1, ty1);
            }
#pragma unroll
            for (int u = 0; u < DET_UNROLL; ++u) {
                if (r0 + u < kept) {                                     // the same in every lane
                    const float v = real && !((taken >> j) & 1u) ? q[u] : -1.f;
                    const float m = group_max<GW>(v, lane);
                    const u64 eq = __ballot(v == m && v >= 0.f);
                    const unsigned hb = (unsigned)(eq >> shift) & (GW == 16 ? 0xffffu : 0xffffffffu);
                    if (hb != 0u && m >= th) {
                        taken |= 1u << __builtin_ctz(hb);
                        ++ntp;
                        if (j == 0) atomicOr(&s_tp[r0 + u], 1 << t);
                    }
                }
            }
        }
        if (j == 0 && active) s_cnt[t] = ntp;
    }
    __syncthreads();

    const size_t row = (size_t)b * max_det;
    for (int r = tid; r < max_det; r += DET_THREADS) {
        const bool on = r < kept;
        const int n = on ? (int)~(unsigned)s_key[r] : -1;
        score_out[row + r] = on ? sc[n] : -__builtin_inff();
        tp_out[row + r] = on ? s_tp[r] : 0;
        order_out[row + r] = n;
    }
    if (tid == 0) {
        n_pred_out[b] = n_pred;
        n_truth_out[b] = cnt;
        const int d = n_pred - cnt;
        if (cnt) atomicAdd(&counters[0], (u64)cnt);
        if (kept) atomicAdd(&counters[1], (u64)kept);
        if (d == 0) atomicAdd(&counters[2], 1ull);
        if (d) {
            atomicAdd(&counters[3], (u64)(d < 0 ? -d : d));
            atomicAdd(&counters[4], (u64)(long long)d);                  // two's complement: the sum is exact in 64 bits
        }
        atomicAdd(&counters[5], 1ull);
    }
    if (tid < T && s_cnt[tid]) atomicAdd(&counters[8 + tid], (u64)s_cnt[tid]);
}

// Exclusive scan over the 1024 threads in thread order (and the total over all of them), for an associative op with identity `ident`
template <class V, class Op>
__device__ __forceinline__ V det_scan(V v, V ident, V* lds, V& total, Op op) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    V x = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const V y = __shfl_up(x, o, 64);
        if (lane >= o) x = op(y, x);
    }
    __syncthreads();                                                     // the previous use of lds is over
    if (lane == 63) lds[wave] = x;
    __syncthreads();
    V pre = ident, all = ident;
#pragma unroll
    for (int w = 0; w < DET_AP_WAVES; ++w) {
        const V s = lds[w];
        if (w < wave) pre = op(pre, s);
        all = op(all, s);
    }
    total = all;
    const V below = __shfl_up(x, 1, 64);
    return lane ? op(pre, below) : pre;
}

__global__ __launch_bounds__(DET_AP_THREADS) void k_det_ap(const int* __restrict__ tp, long long M, int T,
                                                           const long long* __restrict__ counters, double* __restrict__ out) {
    __shared__ int s_i[DET_AP_WAVES];
    __shared__ double s_d[DET_AP_WAVES];
    const int tid = threadIdx.x, t = blockIdx.x;
    const long long NT = counters[0];
    const long long R = min(max(counters[1], 0ll), M);                    // valid records: the slots past them are dead
    const long long TPtot = counters[8 + t];
    double acc = 0.0;
    long long carry_bits = 0;                                            // true positives behind the chunk
    double carry_max = 0.0;                                              // largest precision behind the chunk
    int word[DET_AP_PER];                                                // the chunk's tp words, loaded one chunk ahead
#pragma unroll
    for (int q = 0; q < DET_AP_PER; ++q) {
        const long long i = R - 1 - (long long)tid * DET_AP_PER - q;
        word[q] = i >= 0 ? tp[i] : 0;
    }
    for (long long hi = R; hi > 0; hi -= DET_AP_CHUNK) {
        // thread tid holds the records hi - 1 - (4 tid + q), q = 0 .. 3: position 0 is the last record
        const long long i0 = hi - 1 - (long long)tid * DET_AP_PER;
        int bit[DET_AP_PER], c = 0;
#pragma unroll
        for (int q = 0; q < DET_AP_PER; ++q) {
            bit[q] = (word[q] >> t) & 1;
            c += bit[q];
            const long long i = i0 - q - DET_AP_CHUNK;                   // the same records of the next chunk
            word[q] = i >= 0 ? tp[i] : 0;
        }
        int chunk_bits;
        const int before = det_scan(c, 0, s_i, chunk_bits, [](int a, int b) { return a + b; });
        double prec[DET_AP_PER], m = 0.0;
        long long behind = carry_bits + before;                          // true positives strictly behind record i0 - q
#pragma unroll
        for (int q = 0; q < DET_AP_PER; ++q) {
            const long long i = i0 - q;
            prec[q] = i >= 0 ? (double)(int)(TPtot - behind) / (double)(int)(i + 1) : 0.0;       // (both below 2^31: M_slots is)
            behind += bit[q];
            m = fmax(m, prec[q]);
        }
        double chunk_max;
        double env = fmax(carry_max, det_scan(m, 0.0, s_d, chunk_max, [](double a, double b) { return fmax(a, b); }));
#pragma unroll
        for (int q = 0; q < DET_AP_PER; ++q) {
            env = fmax(env, prec[q]);
            if (bit[q]) acc += env;
        }
        carry_bits += chunk_bits;
        carry_max = fmax(carry_max, chunk_max);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);       // a fixed tree over the lanes, then the waves in order
    __syncthreads();
    if ((tid & 63) == 0) s_d[tid >> 6] = acc;
    __syncthreads();
    if (tid == 0) {
        double s = 0.0;
        for (int w = 0; w < DET_AP_WAVES; ++w) s += s_d[w];
        const double nan = __builtin_nan("");
        out[t] = NT > 0 ? s / (double)NT : nan;
        out[T + t] = NT > 0 ? (double)TPtot / (double)NT : nan;
        out[2 * T + t] = R > 0 ? (double)TPtot / (double)R : nan;
    }
}

}  // namespace

extern "C" int spair_det_match(const float* boxes, const float* scores, const float* bbox, const int* count, const float* thresholds, int B,
                               int N, int K, int T, float min_score, int max_det, float* score, int* tp, int* order, int* n_pred,
                               int* n_truth, long long* counters, float* iou, void* stream) {
    if (B < 1 || N < 1 || N > DET_MAX_N || K < 1 || K > DET_MAX_K || T < 1 || T > DET_MAX_T || max_det < 1 || max_det > N) return SPAIR_ERR_SHAPE;
    if (!(min_score - min_score == 0.f)) return SPAIR_ERR_SHAPE;          // NaN or infinite
    if (!boxes || !scores || !bbox || !count || !thresholds || !score || !tp || !order || !n_pred || !n_truth || !counters) return SPAIR_ERR_SHAPE;
    if (K <= 16)
        hipLaunchKernelGGL(k_det_match<16>, dim3(B), dim3(DET_THREADS), 0, (hipStream_t)stream, boxes, scores, bbox, count, thresholds, N, K, T,
                           min_score, max_det, score, tp, order, n_pred, n_truth, reinterpret_cast<u64*>(counters), iou);
    else
        hipLaunchKernelGGL(k_det_match<32>, dim3(B), dim3(DET_THREADS), 0, (hipStream_t)stream, boxes, scores, bbox, count, thresholds, N, K, T,
                           min_score, max_det, score, tp, order, n_pred, n_truth, reinterpret_cast<u64*>(counters), iou);
    SPAIR_CHECK_LAUNCH();
    return SPAIR_OK;
}

extern "C" int spair_det_ap(const int* tp_sorted, long long M, int T, const long long* counters, double* out, void* stream) {
    if (M < 1 || M > 0x7fffffffLL || T < 1 || T > DET_MAX_T || !tp_sorted || !counters || !out) return SPAIR_ERR_SHAPE;
    hipLaunchKernelGGL(k_det_ap, dim3(T), dim3(DET_AP_THREADS), 0, (hipStream_t)stream, tp_sorted, M, T, counters, out);
    SPAIR_CHECK_LAUNCH();
    return SPAIR_OK;
}
