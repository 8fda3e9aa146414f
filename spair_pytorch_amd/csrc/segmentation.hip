// Segmentation metrics on the device: a predicted label map (the scene parse's per-pixel owners) scored against a true one (the scene
// generator's instance masks).  Adjusted Rand index over all pixels and over the pixels of true objects, segmentation covering
// (unweighted and weighted by object size), foreground IoU; definitions in include/spair_hip.h, "segmentation metrics".
//
// Everything is derived from the contingency table n[i][j] of one image ((NP + 1) x (K + 1) ints, index 0 = background), so the work is
//   k_seg_count:  grid B x S; workgroup (b, s) counts slice s of image b's pixels into a table in LDS and adds the table's non-zero
//                 entries to the image's table in memory with integer atomics (order-independent: bit-identical from run to run);
//   k_seg_finish: one workgroup per image; row / column sums, the sums of C2, the best match of every object, the five scores.
//
// k_seg_count.  A lane takes four consecutive pixels of both maps, 16 bytes per load, where every plane starts 16-byte aligned (HW a
// multiple of 4 and aligned bases), otherwise one pixel; consecutive lanes on consecutive units.  Around 90 % of a scene is background on
// both sides: those pixels never touch LDS, a lane counts them in a register and the wave adds its total once.  The other pixels lie in
// regions (neighbouring pixels belong to the same object and the same cell), and same-address LDS atomics serialise, so equal pairs are
// merged before they reach LDS: a lane whose four pixels share a pair holds one count of 4; consecutive lanes with the same pair form a
// run (one shuffle and one ballot find them) and the run's first lane issues one atomic for all of it.  Only a lane that straddles a
// boundary adds its pixels one by one.  (A first version took the wave's distinct pairs one at a time, a ballot each: a 256-pixel row
// of a 32 x 32-cell parse holds 32 of them, and the loop, not memory, set the time -- 161 us against 59 at 16 x 16 cells.)
//
// The split (seg_slices), as evaluate.hip's: S = ceil(2048 / B) workgroups per image, but never fewer than four pixels per lane in a
// slice, and never so many that clearing and scanning the tables outweighs the pixels: a slice holds at least half as many pixels as the
// table has entries (the table is cleared and scanned 16 bytes per lane).  At NP = 1024, K = 32 the table is 135,312 bytes: one
// workgroup per CU.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <atomic>

#include "common.h"

namespace {

constexpr int SEG_MAX_NP = 1024;
constexpr int SEG_MAX_K = 32;                     // SC_MAXOBJ of scenes.hip
constexpr long long SEG_MAX_HW = 1ll << 24;
constexpr int SEG_TARGET_BLOCKS = 2048;
constexpr int SEG_MAX_LDS = ((SEG_MAX_NP + 1) * (SEG_MAX_K + 1) + 3) / 4 * 16;       // 135,312 bytes: inside the CU's 160 KiB

typedef unsigned long long u64;
typedef unsigned __int128 u128;
typedef __int128 i128;

// Lanes that hold `w` pixels of one pair `idx` each (on; idx > 0) into the table: consecutive lanes with the same pair form a run, and
// the run's first lane adds the whole run with one LDS atomic.  Called by all 64 lanes together; no loop.
__device__ __forceinline__ void seg_add_runs(bool on, int idx, int w, int lane, int* __restrict__ tab) {
    const int key = on ? idx : -1;
    const int before = __shfl_up(key, 1, 64);
    const bool follows = on && lane > 0 && before == idx;                 // continues the run of the lane below
    const u64 f = __ballot(follows);
    if (on && !follows) {
        const u64 above = lane == 63 ? 0ull : f >> (lane + 1);            // the run: the consecutive followers above this lane
        atomicAdd(&tab[idx], w * (1 + (int)__builtin_ctzll(~above)));
    }
}

__device__ __forceinline__ int seg_index(int p, int t, int NP, int K) {
    const int pi = (unsigned)p < (unsigned)NP ? p + 1 : 0;        // below -1, or at or above the count: background
    const int ti = (unsigned)t < (unsigned)K ? t + 1 : 0;
    return pi * (K + 1) + ti;
}

template <bool VEC>
__global__ __launch_bounds__(256) void k_seg_count(const int* __restrict__ pred, const int* __restrict__ truth, long long HW, int NP, int K, int S,
                                                   long long units_per, int* __restrict__ contingency) {
    extern __shared__ int4 tab4[];                                 // the table, padded to a multiple of four entries
    int* tab = reinterpret_cast<int*>(tab4);
    const int tid = threadIdx.x, lane = tid & 63;
    const int b = blockIdx.x / S, s = blockIdx.x % S;
    const int T = (NP + 1) * (K + 1), T4 = (T + 3) >> 2;
    for (int e = tid; e < T4; e += 256) tab4[e] = make_int4(0, 0, 0, 0);
    __syncthreads();
    const int* pp = pred + (size_t)b * HW;
    const int* tp = truth + (size_t)b * HW;
    const long long nunits = VEC ? HW / 4 : HW;
    const long long u0 = (long long)s * units_per, u1 = min(u0 + units_per, nunits);
    int nbg = 0;
    for (long long base = u0; base < u1; base += 256) {          // wave-uniform trip count: every lane reaches the shuffle and the ballot
        const long long u = base + tid;
        const bool ok = u < u1;
        if (VEC) {
            int4 p = make_int4(0, 0, 0, 0), t = make_int4(0, 0, 0, 0);
            if (ok) {
                p = *reinterpret_cast<const int4*>(pp + 4 * u);
                t = *reinterpret_cast<const int4*>(tp + 4 * u);
            }
            const int i0 = seg_index(p.x, t.x, NP, K), i1 = seg_index(p.y, t.y, NP, K), i2 = seg_index(p.z, t.z, NP, K),
                      i3 = seg_index(p.w, t.w, NP, K);
            const bool one = ok && i0 == i1 && i0 == i2 && i0 == i3;       // the lane's four pixels on one pair: the rule inside a region
            if (one && i0 == 0) nbg += 4;
            seg_add_runs(one && i0 > 0, i0, 4, lane, tab);
            if (ok && !one) {                                               // a lane across a boundary: pixel by pixel
                if (i0) atomicAdd(&tab[i0], 1); else ++nbg;
                if (i1) atomicAdd(&tab[i1], 1); else ++nbg;
                if (i2) atomicAdd(&tab[i2], 1); else ++nbg;
                if (i3) atomicAdd(&tab[i3], 1); else ++nbg;
            }
        } else {
            int p = 0, t = 0;
            if (ok) { p = pp[u]; t = tp[u]; }
            const int i = seg_index(p, t, NP, K);
            if (ok && i == 0) ++nbg;
            seg_add_runs(ok && i > 0, i, 1, lane, tab);
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) nbg += __shfl_xor(nbg, o, 64);
    if (lane == 0 && nbg) atomicAdd(&tab[0], nbg);
    __syncthreads();
    int* out = contingency + (size_t)b * T;
    for (int e = tid; e < T4; e += 256) {                        // (entries T .. 4 T4 - 1 are never counted into: they stay 0)
        const int4 v = tab4[e];
        if (v.x | v.y | v.z | v.w) {
            if (v.x) atomicAdd(&out[4 * e], v.x);
            if (v.y) atomicAdd(&out[4 * e + 1], v.y);
            if (v.z) atomicAdd(&out[4 * e + 2], v.z);
            if (v.w) atomicAdd(&out[4 * e + 3], v.w);
        }
    }
}

__device__ __forceinline__ u64 c2(u64 v) { return v * (v - 1) / 2; }       // v = 0: 0 * (2^64 - 1) / 2 = 0

constexpr int SEG_FIN_THREADS = 1024;             // k_seg_finish: 16 waves walk one image's table (up to 33,825 entries)
constexpr int SEG_FIN_WAVES = SEG_FIN_THREADS / 64;

// Sum over the block of k_seg_finish, result in every thread (integers: the order does not matter)
__device__ __forceinline__ u64 block_sum_u64(u64 v, u64* red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += (u64)__shfl_xor((long long)v, o, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    u64 t = 0;
#pragma unroll
    for (int w = 0; w < SEG_FIN_WAVES; ++w) t += red[w];
    return t;
}

__device__ __forceinline__ double u128_to_double(u128 v) {
    return (double)(u64)(v >> 64) * 18446744073709551616.0 + (double)(u64)v;
}

// (X - E) / (M - E) of the header from the integer sums: 2 (X C - A Bs) / ((A + Bs) C - 2 A Bs) with C = C2(N), both exact in 128 bits
// (X, A, Bs, C < 2^48); a zero denominator -- decided on the integers -- gives 1.
__device__ double seg_ari(u64 X, u64 A, u64 Bs, u64 C) {
    const u128 ab = (u128)A * Bs;
    const i128 num = 2 * ((i128)((u128)X * C) - (i128)ab);
    const i128 den = (i128)((u128)(A + Bs) * C) - 2 * (i128)ab;
    if (den == 0) return 1.0;
    const double n = num < 0 ? -u128_to_double((u128)(-num)) : u128_to_double((u128)num);
    return n / u128_to_double((u128)den);         // M >= E: den > 0
}

// is candidate (n1 / u1, label i1) a better match than (n2 / u2, i2)?  n = 0: no candidate.  Cross-multiplied: n < 2^24 + 1, u < 2^25 + 1.
__device__ __forceinline__ bool seg_better(int n1, int u1, int i1, int n2, int u2, int i2) {
    const u64 l = (u64)n1 * (u64)u2, r = (u64)n2 * (u64)u1;
    return l > r || (l == r && n1 > 0 && i1 < i2);
}

__global__ __launch_bounds__(SEG_FIN_THREADS) void k_seg_finish(const int* __restrict__ contingency, long long HW, int NP, int K, float* __restrict__ scores,
                                                    int* __restrict__ match, float* __restrict__ match_iou) {
    __shared__ int s_row[SEG_MAX_NP + 1];
    __shared__ int s_col[SEG_MAX_K + 1];
    __shared__ int s_bn[SEG_MAX_K + 1], s_bu[SEG_MAX_K + 1];
    __shared__ u64 red[SEG_FIN_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.x, K1 = K + 1, T = (NP + 1) * K1;
    const int* n = contingency + (size_t)b * T;
    for (int i = tid; i <= NP; i += SEG_FIN_THREADS) s_row[i] = 0;
    if (tid <= K) s_col[tid] = 0;
    __syncthreads();
    // row and column sums (LDS integer atomics on the non-zero entries: a parse's table is sparse), sum C2(n_ij) over all columns and
    // over the object columns
    u64 x_all = 0, x_fg = 0;
    for (int e = tid; e < T; e += SEG_FIN_THREADS) {
        const int v = n[e];
        if (v) {
            const int i = e / K1, j = e - i * K1;
            atomicAdd(&s_row[i], v);
            atomicAdd(&s_col[j], v);
            const u64 c = c2((u64)v);
            x_all += c;
            if (j) x_fg += c;
        }
    }
    __syncthreads();
    u64 a_all = 0, a_fg = 0;
    for (int i = tid; i <= NP; i += SEG_FIN_THREADS) {
        const u64 a = (u64)s_row[i];
        a_all += c2(a);
        a_fg += c2(a - (u64)n[(size_t)i * K1]);
    }
    x_all = block_sum_u64(x_all, red);
    x_fg = block_sum_u64(x_fg, red);
    a_all = block_sum_u64(a_all, red);
    a_fg = block_sum_u64(a_fg, red);
    // best match of every object: a wave per column, lanes over the predicted segments, the triple (n, union, label) reduced by shuffles
    for (int j = 1 + wave; j <= K; j += SEG_FIN_WAVES) {
        const int bj = s_col[j];
        int bn = 0, bu = 1, bi = 0x7fffffff;
        if (bj > 0) {
            for (int i = 1 + lane; i <= NP; i += 64) {
                const int v = n[(size_t)i * K1 + j];
                const int u = s_row[i] + bj - v;
                if (v > 0 && seg_better(v, u, i, bn, bu, bi)) { bn = v; bu = u; bi = i; }
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                const int on = __shfl_xor(bn, o, 64), ou = __shfl_xor(bu, o, 64), oi = __shfl_xor(bi, o, 64);
                if (seg_better(on, ou, oi, bn, bu, bi)) { bn = on; bu = ou; bi = oi; }
            }
        }
        if (lane == 0) {
            s_bn[j] = bn; s_bu[j] = bu;
            if (match) match[(size_t)b * K + j - 1] = bn > 0 ? bi - 1 : -1;
            if (match_iou) match_iou[(size_t)b * K + j - 1] = (float)((double)bn / (double)bu);
        }
    }
    __syncthreads();
    if (tid == 0) {
        const u64 N = (u64)HW, b0 = (u64)s_col[0], a0 = (u64)s_row[0], n00 = (u64)n[0];
        u64 b_all = 0, b_fg = 0;
        for (int j = 0; j <= K; ++j) {
            const u64 c = c2((u64)s_col[j]);
            b_all += c;
            if (j) b_fg += c;
        }
        const u64 Nf = N - b0;
        double msc = 0.0, sc = 0.0;
        int nobj = 0;
        for (int j = 1; j <= K; ++j) {                     // fixed order
            if (s_col[j] > 0) {
                const double q = (double)s_bn[j] / (double)s_bu[j];
                msc += q;
                sc += (double)s_col[j] * q;
                ++nobj;
            }
        }
        const float nan = __builtin_nanf("");
        float* o = scores + (size_t)b * 5;
        o[0] = (float)seg_ari(x_all, a_all, b_all, c2(N));
        o[1] = Nf ? (float)seg_ari(x_fg, a_fg, b_fg, c2(Nf)) : nan;
        o[2] = nobj ? (float)(msc / (double)nobj) : nan;
        o[3] = nobj ? (float)(sc / (double)Nf) : nan;
        const u64 uni = N - n00, inter = N + n00 - a0 - b0;
        o[4] = uni ? (float)((double)inter / (double)uni) : 1.f;
    }
}

int seg_slices(int B, long long HW, int T) {
    const long long by_work = (HW + 1023) / 1024;                       // four pixels per lane
    const long long by_table = 2 * HW / T;                              // a slice: at least T / 2 pixels
    const long long want = (SEG_TARGET_BLOCKS + (long long)B - 1) / B;
    return (int)std::max<long long>(1, std::min(std::min(want, by_work), by_table));
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

std::atomic<unsigned long long> g_lds_vec{0}, g_lds_one{0};

}  // namespace

extern "C" int spair_segmentation(const int* pred, const int* truth, int B, long long HW, int NP, int K, int* contingency, float* scores,
                                  int* match, float* match_iou, void* stream) {
    if (B < 1 || HW < 1 || HW > SEG_MAX_HW || NP < 1 || NP > SEG_MAX_NP || K < 1 || K > SEG_MAX_K) return SPAIR_ERR_SHAPE;
    if (!pred || !truth || !contingency || !scores) return SPAIR_ERR_SHAPE;
    hipStream_t s = (hipStream_t)stream;
    const int T = (NP + 1) * (K + 1);
    const int S = seg_slices(B, HW, T);
    if ((long long)B * S > 0x7fffffffLL) return SPAIR_ERR_UNSUPPORTED;
    const bool vec = HW % 4 == 0 && aligned16(pred) && aligned16(truth);
    const long long nunits = vec ? HW / 4 : HW;
    const long long units_per = (nunits + S - 1) / S;
    const int lds = (T + 3) / 4 * 16;
    const void* fn = vec ? reinterpret_cast<const void*>(&k_seg_count<true>) : reinterpret_cast<const void*>(&k_seg_count<false>);
    if (lds > 64 * 1024) {                                            // above the default cap on dynamic LDS
        const int rc = spair_dyn_lds_once(fn, SEG_MAX_LDS, vec ? g_lds_vec : g_lds_one);
        if (rc != SPAIR_OK) return rc;
    }
    if (hipMemsetAsync(contingency, 0, (size_t)B * T * sizeof(int), s) != hipSuccess) return SPAIR_ERR_LAUNCH;
    const dim3 grid((unsigned)(B * S)), block(256);
    if (vec)
        hipLaunchKernelGGL((k_seg_count<true>), grid, block, lds, s, pred, truth, HW, NP, K, S, units_per, contingency);
    else
        hipLaunchKernelGGL((k_seg_count<false>), grid, block, lds, s, pred, truth, HW, NP, K, S, units_per, contingency);
    SPAIR_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_seg_finish, dim3(B), dim3(SEG_FIN_THREADS), 0, s, contingency, HW, NP, K, scores, match, match_iou);
    SPAIR_CHECK_LAUNCH();
    return SPAIR_OK;
}
