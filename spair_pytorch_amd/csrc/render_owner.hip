// The scene parse's per-pixel owner map: the renderer's gather (reference: models.py:511-537, stn(inverse=True) modules.py:256-269) done
// once, keeping the ARG-MAX of the composite's per-object coefficients instead of their colour-weighted sum.  For sample b, pixel (y, x)
// and cell k = h * Gw + w (row-major grid order):
//     a_k = warp(alpha_k * pres_k),  m_k = warp(max(alpha_k * pres_k * depth_k, 0.01))   (bilinear, taps on the padding are zero)
//     D   = sum_k m_k + HW * 1e-9
//     w_k = a_k (m_k + 1e-9) / D          -- the coefficient of object k's colour in the composite (render.hip: num += g * a * (m + 1e-9))
//     coverage = sum_k w_k,  owner_weight = max_k w_k,  owner = the smallest k that reaches it (or -1: nothing, or below the threshold),
//     area[b][k] = pixels of sample b owned by k.
// D is common to a pixel's objects, so the kernel keeps the running best of u_k = a_k (m_k + 1e-9) and divides once.
//
// Structure: k_render_fwd's (render.hip) -- one workgroup per (sample, 16 x 16 tile), the HW objects culled in chunks of 256 into an LDS
// list by ballot compaction with the finer per-wave (16 x 4 strip) lists, the branch-free tap loop with the next candidate's four loads in
// flight, all tiles of a sample on one XCD.  What differs:
//   * the chunk is walked in ROW-MAJOR cell order k and reads row cidx[k] * B + b (the step's rows are in dependency-wavefront order);
//     the ballot compaction keeps the order, so "a strictly larger u replaces the best" is the lowest-k tie rule for free;
//   * a tap loads the alpha element alone: texel stride CH = C + 1 elements of fp16 or fp32, alpha last -- the grey (grey, alpha) pairs,
//     the colour [P*P][C+1] sprites and the conv decoder's fp32 sprites are one kernel;
//   * no logarithm, no image read; owner / owner_weight / coverage are 12 bytes per pixel;
//   * the areas are counted in an LDS histogram per workgroup and flushed with one integer atomic per (workgroup, owning cell): exact and
//     order-independent, so every output is bit-identical from run to run.  No float atomics.
// 72 VGPRs, no scratch: 7 waves per SIMD (k_render_fwd: 75 - 77, 6 waves).  Measured and rejected: fetching the next chunk's table entry a
// chunk ahead together with a compile-time texel stride of 2 -- 74 VGPRs, 6 waves per SIMD, and 5 - 8 % slower at both benchmark
// geometries: the seventh wave is worth more than the dependent load it hides.
#include "render_common.h"

namespace {

struct OCand {                 // 32 bytes: two ds_read_b128
    float ax, bx, ay, by, pres, pd;
    int row, k;
};

constexpr int RO_MAXHW = 1024;  // cells per sample (the step's own limit: cells_init_tables)

template <bool S16>
__device__ __forceinline__ float ld_alpha(const float* __restrict__ S, size_t e) {
    if constexpr (S16) return (float)reinterpret_cast<const _Float16*>(S)[e];
    else return S[e];
}

template <bool S16>
__global__ __launch_bounds__(256) void k_render_owner(const float* __restrict__ S, int ld_s, int CH, const float* __restrict__ nbox,
                                                      const float* __restrict__ pres, const float* __restrict__ depth, int ld_pd,
                                                      const int* __restrict__ cidx, float threshold, int* __restrict__ owner,
                                                      float* __restrict__ owner_weight, float* __restrict__ coverage,
                                                      int* __restrict__ area, int B, int HW, int I, int Iw, int P, int ac) {
    __shared__ OCand cand[RCH];
    __shared__ unsigned short wlist[4][RCH];     // per wave (= a 16 x 4 pixel strip of the tile): the candidates that reach its rows
    __shared__ int wave_cnt[4][5];               // [culling wave][tile, strip 0..3]
    __shared__ int hist[RO_MAXHW];               // pixels of this tile per owning cell
    const int tiles_x = (Iw + RT - 1) / RT, tiles = tiles_x * ((I + RT - 1) / RT);     // canvas I rows x Iw columns
    int b, tile;
    if ((B & 7) == 0) {   // XCD-aware: blocks id, id+8, ... share an XCD (round-robin dispatch)
        const int xcd = blockIdx.x & 7, j = blockIdx.x >> 3;
        b = (j / tiles) * 8 + xcd;
        tile = j % tiles;
    } else {
        b = blockIdx.x / tiles;
        tile = blockIdx.x % tiles;
    }
    const int tx0 = (tile % tiles_x) * RT, ty0 = (tile / tiles_x) * RT;
    const int lx = threadIdx.x & (RT - 1), ly = threadIdx.x >> 4;
    const int px = tx0 + lx, py = ty0 + ly;
    const bool inside = px < Iw && py < I;
    const int tx1 = min(tx0 + RT, Iw) - 1, ty1 = min(ty0 + RT, I) - 1;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int e = threadIdx.x; e < HW; e += 256) hist[e] = 0;      // (the chunk loop's barriers order it before the counting)

    float best = 0.f, sum_u = 0.f, den = 0.f;
    int best_k = -1;
    const float bX = stn_base(min(px, Iw - 1), Iw, ac), bY = stn_base(min(py, I - 1), I, ac);   // this pixel's base coordinate, once
    for (int k0 = 0; k0 < HW; k0 += RCH) {
        // ---- cull RCH objects, in row-major cell order, against this tile
        const int k = k0 + threadIdx.x;
        bool hit = false;
        OCand c;
        if (k < HW) {
            const int cp = cidx ? cidx[k] : k;
            if (cp >= 0 && cp < HW) {        // (a table entry outside the rows is no object)
                const int r = cp * B + b;
                const float4 nb = *reinterpret_cast<const float4*>(nbox + (size_t)r * 4);
                const float tx = 2.f * nb.x - 1.f, ty = 2.f * nb.y - 1.f;
                c.ax = 1.f / nb.z; c.bx = -tx / nb.z; c.ay = 1.f / nb.w; c.by = -ty / nb.w;
                c.pres = pres[(size_t)r * ld_pd]; c.pd = c.pres * depth[(size_t)r * ld_pd]; c.row = r; c.k = k;
                // the zero-padded sprite is non-zero for source coords in (-1, P)
                hit = src_of(c.ax, c.bx, tx1, Iw, P, ac) > -1.f && src_of(c.ax, c.bx, tx0, Iw, P, ac) < (float)P &&
                      src_of(c.ay, c.by, ty1, I, P, ac) > -1.f && src_of(c.ay, c.by, ty0, I, P, ac) < (float)P;
            }
        }
        // the finer cull per wave strip (render.hip): skipped pairs have zero weights, so nothing changes to the bit
        bool hs[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int sy0 = ty0 + 4 * q, sy1 = min(sy0 + 3, I - 1);
            hs[q] = hit && sy0 < I && src_of(c.ay, c.by, sy1, I, P, ac) > -1.f && src_of(c.ay, c.by, sy0, I, P, ac) < (float)P;
        }
        const unsigned long long bal = __ballot(hit);
        unsigned long long bs[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) bs[q] = __ballot(hs[q]);
        if (lane == 0) {
            wave_cnt[wave][0] = __popcll(bal);
#pragma unroll
            for (int q = 0; q < 4; ++q) wave_cnt[wave][1 + q] = __popcll(bs[q]);
        }
        __syncthreads();
        int base = 0;
        for (int w = 0; w < wave; ++w) base += wave_cnt[w][0];
        const unsigned long long below = (1ull << lane) - 1ull;
        const int ci_me = base + __popcll(bal & below);
        if (hit) cand[ci_me] = c;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            int bq = 0;
            for (int w = 0; w < wave; ++w) bq += wave_cnt[w][1 + q];
            if (hs[q]) wlist[q][bq + __popcll(bs[q] & below)] = (unsigned short)ci_me;
        }
        __syncthreads();
        const int nc = wave_cnt[0][1 + wave] + wave_cnt[1][1 + wave] + wave_cnt[2][1 + wave] + wave_cnt[3][1 + wave];
        const unsigned short* const wl = wlist[wave];
        // ---- the surviving objects at this thread's pixel, ascending k.  Branch-free and software-pipelined as k_render_fwd: the four
        // alpha taps of candidate ci+1 are in flight while candidate ci is weighed (taps outside the sprite / pixels the object does not
        // cover read a clamped texel with weight 0).
        if (inside && nc > 0) {
            float tv[4], tn[4], tw[4], twn[4];
            float prs = 0.f, pdd = 0.f, prs_n = 0.f, pdd_n = 0.f;
            int kk = 0, kk_n = 0;
            auto fetch = [&](int ci, float (&v)[4], float (&w)[4], float& pr_, float& pd_, int& k_) {
                const OCand q = cand[ci];
                float gdum;
                const float sx = src_from_base(q.ax, q.bx, bX, P, ac, gdum), sy = src_from_base(q.ay, q.by, bY, P, ac, gdum);
                const bool cov = sx > -1.f && sx < (float)P && sy > -1.f && sy < (float)P;
                const float fx = floorf(sx), fy = floorf(sy);
                const int x0 = (int)fminf(fmaxf(fx, -1.f), (float)(P - 1)), y0 = (int)fminf(fmaxf(fy, -1.f), (float)(P - 1));
                const float wx1 = sx - fx, wy1 = sy - fy, wx0 = 1.f - wx1, wy0 = 1.f - wy1;
                const size_t sp = (size_t)q.row * ld_s + (CH - 1);      // the alpha element of the sprite's first texel
                pr_ = q.pres; pd_ = q.pd; k_ = q.k;
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    const int yy = y0 + (t >> 1), xx = x0 + (t & 1);
                    const bool ok = cov && yy >= 0 && yy < P && xx >= 0 && xx < P;
                    w[t] = ok ? ((t >> 1) ? wy1 : wy0) * ((t & 1) ? wx1 : wx0) : 0.f;
                    v[t] = ld_alpha<S16>(S, sp + (size_t)((min(max(yy, 0), P - 1) * P + min(max(xx, 0), P - 1)) * CH));
                }
            };
            fetch(wl[0], tv, tw, prs, pdd, kk);
            for (int ci = 0; ci < nc; ++ci) {
                fetch(wl[min(ci + 1, nc - 1)], tn, twn, prs_n, pdd_n, kk_n);
                float a = 0.f, m = 0.f;
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    a += tw[t] * (tv[t] * prs);
                    m += tw[t] * fmaxf(tv[t] * pdd, 0.01f);
                }
                const float u = a * (m + 1e-9f);
                sum_u += u;
                den += m;
                if (u > best) { best = u; best_k = kk; }      // ascending k: the first maximum stays
#pragma unroll
                for (int t = 0; t < 4; ++t) { tv[t] = tn[t]; tw[t] = twn[t]; }
                prs = prs_n; pdd = pdd_n; kk = kk_n;
            }
        }
        __syncthreads();
    }
    if (inside) {
        const float D = den + (float)HW * 1e-9f;   // every object adds 1e-9 (models.py:527)
        const float invD = 1.f / D;
        const float wbest = best * invD;
        const int own = (wbest > 0.f && wbest >= threshold) ? best_k : -1;
        const size_t pi = ((size_t)b * I + py) * Iw + px;
        owner[pi] = own;
        owner_weight[pi] = wbest;
        coverage[pi] = sum_u * invD;
        if (own >= 0) atomicAdd(&hist[own], 1);
    }
    __syncthreads();
    for (int e = threadIdx.x; e < HW; e += 256) {
        const int n = hist[e];
        if (n) atomicAdd(area + (size_t)b * HW + e, n);
    }
}

}  // namespace

// owner [B][I][Iw] int32, owner_weight / coverage [B][I][Iw] fp32, area [B][HW] int32 (zeroed here); cidx: HW ints (cell k -> row block,
// rows cidx[k] * B + b) or null = identity; CH = elements per texel (alpha last), s16: fp16 sprites, ld_s in elements of that type
int render_owner(const RenderGeom& g, const float* S, int ld_s, int s16, int CH, const int* cidx, float threshold, int* owner,
                 float* owner_weight, float* coverage, int* area, hipStream_t s) {
    if (g.B <= 0 || g.HW <= 0 || g.I <= 0 || g.Iw <= 0 || g.P < 1 || CH < 2 || ld_s < g.P * g.P * CH) return SPAIR_ERR_SHAPE;
    if (g.HW > RO_MAXHW || (long long)g.B * g.I * g.Iw > 0x7fffffffLL) return SPAIR_ERR_UNSUPPORTED;
    if (hipMemsetAsync(area, 0, (size_t)g.B * g.HW * sizeof(int), s) != hipSuccess) return SPAIR_ERR_LAUNCH;
    hipLaunchKernelGGL(s16 ? k_render_owner<true> : k_render_owner<false>, dim3(render_num_blocks(g.B, g.I, g.Iw)), dim3(256), 0, s, S, ld_s,
                       CH, g.nbox, g.pres, g.depth, g.ld_pd, cidx, threshold, owner, owner_weight, coverage, area, g.B, g.HW, g.I, g.Iw, g.P,
                       g.ac);
    SPAIR_CHECK_LAUNCH();
    return SPAIR_OK;
}

// unit-level C ABI: rows r = (cidx ? cidx[k] : k) * B + b of sprites [N][ld_s], nbox [N][4], pres [N], depth [N]
extern "C" int spair_render_owner(const void* sprites, int ld_s, int s16, int ch, const float* nbox, const float* pres, const float* depth,
                                  const int* cidx, float threshold, int* owner, float* owner_weight, float* coverage, int* area, int B,
                                  int HW, int I, int Iw, int P, int align_corners, void* stream) {
    if (!sprites || !nbox || !pres || !depth || !owner || !owner_weight || !coverage || !area) return SPAIR_ERR_SHAPE;
    return render_owner({nbox, pres, depth, 1, B, HW, I, P, align_corners, Iw}, reinterpret_cast<const float*>(sprites), ld_s, s16, ch, cidx,
                        threshold, owner, owner_weight, coverage, area, (hipStream_t)stream);
}
