// SPAIR.compose: a scene rendered from GIVEN latents (reference: _render, models.py:452-542, a pure function of z_attr / z_where / z_depth /
// z_pres), and the composite kept per requested object.
//
// k_latents_import -- the inverse of k_export (misc.hip).  One thread per (row r = cprime * B + b, column j < ld_rec), j fastest, so every
//   store is row-contiguous; the loads gather from the NCHW maps.  One pass, no atomics.  Column j of a row carries z_what[j] to Za / Za16
//   (zero for j >= A: the padding the decoder's K loop reads) and to rec[4 + j]; columns A and A + 1 carry the depth and the presence to
//   rec[4 + A], rec[REC - 1] (what RenderGeom points at); columns 0 .. 3 carry z_where to nbox (verbatim: cells.hip, k_box_sample).  Za16
//   is rounded as the per-cell chain and spair_to_bf16 round it: (__bf16) of the fp32 value rec holds.
//
// k_render_layers -- for sample b, pixel (y, x) and each of the K requested cells k (row-major index; anything outside [0, HW): skipped):
//     a_k = warp(alpha_k * pres_k),  m_k = warp(max(alpha_k * pres_k * depth_k, 0.01))     (bilinear, taps on the padding are zero)
//     layer_weight_k = a_k (m_k + 1e-9) / D,   layers_k[c] = layer_weight_k * warp(colour_k[c])
//   with 1/D the value the renderer forward stored per pixel (inv_den; D sums ALL cells), so the sum of the layers of all cells is the
//   composite before its clamp: the product of two warps per object, not the warp of a product (models.py:529).  One workgroup per
//   (sample, 16 x 16 tile) walks the K cells: work is proportional to K, not to G * Gw.  The footprint test, the source coordinate and the
//   four taps are k_render_fwd's / k_render_owner's own (render_common.h, stn_math.h).  Pixels outside a footprint and skipped cells are
//   stored as zeros: the kernel is the only writer of both outputs, nothing is memset.  No atomics: bit-identical from run to run.
//   Sprite element fp16 or fp32, texel stride C + 1, alpha last (grey pairs, colour, the conv decoder's fp32 sprites: one family).
//   The cell's row parameters are workgroup-uniform (scalar loads).  The kernel stores (C + 1) * 4 bytes per (pixel, cell); measured
//   (profiles/f9_compose_kernels.txt): 2.2 - 2.7 TB/s of stores at K = 8, about 40 % of what plain stores
//   reach -- a wave's store covers four 64-byte tile-row segments.  gfx950 resource usage: k_latents_import 18 VGPRs, k_render_layers
//   30 - 42 VGPRs over its six instantiations, no scratch, no LDS, 8 waves per SIMD.
#include "compose.h"
#include "render_common.h"

namespace {

__global__ __launch_bounds__(256) void k_latents_import(CellLayout L, const int* __restrict__ cell_h, const int* __restrict__ cell_w,
                                                        const float* __restrict__ z_where, const float* __restrict__ z_what,
                                                        const float* __restrict__ z_depth, const float* __restrict__ z_pres,
                                                        float* __restrict__ nbox, float* __restrict__ rec, float* __restrict__ Za,
                                                        __bf16* __restrict__ Za16) {
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long long)L.N * L.ld_rec) return;
    const int r = (int)(idx / L.ld_rec), j = (int)(idx - (long long)r * L.ld_rec);
    const int cp = r / L.B, b = r - cp * L.B;
    const size_t cell = (size_t)cell_h[cp] * L.Gw + cell_w[cp], hw = (size_t)L.G * L.Gw;
    float v = 0.f;
    if (j < L.A) {
        v = z_what[((size_t)b * L.A + j) * hw + cell];
        rec[(size_t)r * L.ld_rec + 4 + j] = v;
    } else if (j == L.A) {
        rec[(size_t)r * L.ld_rec + 4 + L.A] = z_depth[(size_t)b * hw + cell];
    } else if (j == L.A + 1) {
        rec[(size_t)r * L.ld_rec + L.REC - 1] = z_pres[(size_t)b * hw + cell];
    }
    Za[idx] = v;
    if (Za16) Za16[idx] = (__bf16)v;
    if (j < 4) nbox[(size_t)r * 4 + j] = z_where[((size_t)b * 4 + j) * hw + cell];
}

template <bool S16>
__device__ __forceinline__ float ld_elem(const float* __restrict__ S, size_t e) {
    if constexpr (S16) return (float)reinterpret_cast<const _Float16*>(S)[e];
    else return S[e];
}

template <bool S16, int C>
__global__ __launch_bounds__(256) void k_render_layers(const float* __restrict__ S, int ld_s, const float* __restrict__ nbox,
                                                       const float* __restrict__ pres, const float* __restrict__ depth, int ld_pd,
                                                       const int* __restrict__ cidx, const int* __restrict__ cells, int K,
                                                       const float* __restrict__ inv_den, float* __restrict__ layers,
                                                       float* __restrict__ layer_weight, int B, int HW, int I, int Iw, int P, int ac) {
    constexpr int CH = C + 1;
    const int tiles_x = (Iw + RT - 1) / RT, tiles = tiles_x * ((I + RT - 1) / RT);     // canvas I rows x Iw columns
    const int b = blockIdx.x / tiles, tile = blockIdx.x % tiles;
    const int tx0 = (tile % tiles_x) * RT, ty0 = (tile / tiles_x) * RT;
    const int px = tx0 + (threadIdx.x & (RT - 1)), py = ty0 + (threadIdx.x >> 4);
    if (px >= Iw || py >= I) return;      // (no barrier below)
    const int tx1 = min(tx0 + RT, Iw) - 1, ty1 = min(ty0 + RT, I) - 1;
    const float bX = stn_base(px, Iw, ac), bY = stn_base(py, I, ac);   // this pixel's base coordinate, once
    const size_t plane = (size_t)I * Iw, pix = (size_t)py * Iw + px;
    const float invD = inv_den[(size_t)b * plane + pix];
    for (int kk = 0; kk < K; ++kk) {
        float wk = 0.f, col[C];
#pragma unroll
        for (int c = 0; c < C; ++c) col[c] = 0.f;
        const int k = cells[(size_t)b * K + kk];
        int cp = -1;
        if (k >= 0 && k < HW) cp = cidx ? cidx[k] : k;
        if (cp >= 0 && cp < HW) {        // (a table entry outside the rows is no object)
            const int r = cp * B + b;
            const float4 nb = *reinterpret_cast<const float4*>(nbox + (size_t)r * 4);
            const float tx = 2.f * nb.x - 1.f, ty = 2.f * nb.y - 1.f;
            const float ax = 1.f / nb.z, bx = -tx / nb.z, ay = 1.f / nb.w, by = -ty / nb.w;
            // the zero-padded sprite is non-zero for source coords in (-1, P): the tile's footprint test, then the pixel's
            const bool hit = src_of(ax, bx, tx1, Iw, P, ac) > -1.f && src_of(ax, bx, tx0, Iw, P, ac) < (float)P &&
                             src_of(ay, by, ty1, I, P, ac) > -1.f && src_of(ay, by, ty0, I, P, ac) < (float)P;
            float gdum;
            const float sx = src_from_base(ax, bx, bX, P, ac, gdum), sy = src_from_base(ay, by, bY, P, ac, gdum);
            if (hit && sx > -1.f && sx < (float)P && sy > -1.f && sy < (float)P) {
                const float prs = pres[(size_t)r * ld_pd], pdd = prs * depth[(size_t)r * ld_pd];
                const float fx = floorf(sx), fy = floorf(sy);
                const int x0 = (int)fminf(fmaxf(fx, -1.f), (float)(P - 1)), y0 = (int)fminf(fmaxf(fy, -1.f), (float)(P - 1));
                const float wx1 = sx - fx, wy1 = sy - fy, wx0 = 1.f - wx1, wy0 = 1.f - wy1;
                const size_t sp = (size_t)r * ld_s;
                float a = 0.f, m = 0.f;
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    const int yy = y0 + (t >> 1), xx = x0 + (t & 1);
                    const bool ok = yy >= 0 && yy < P && xx >= 0 && xx < P;
                    const float w = ok ? ((t >> 1) ? wy1 : wy0) * ((t & 1) ? wx1 : wx0) : 0.f;
                    const size_t e = sp + (size_t)((min(max(yy, 0), P - 1) * P + min(max(xx, 0), P - 1)) * CH);
                    const float al = ld_elem<S16>(S, e + C);
#pragma unroll
                    for (int c = 0; c < C; ++c) col[c] += w * ld_elem<S16>(S, e + c);
                    a += w * (al * prs);
                    m += w * fmaxf(al * pdd, 0.01f);
                }
                wk = a * (m + 1e-9f) * invD;
            }
        }
        const size_t o = (size_t)b * K + kk;
        layer_weight[o * plane + pix] = wk;
#pragma unroll
        for (int c = 0; c < C; ++c) layers[(o * C + c) * plane + pix] = wk * col[c];
    }
}

}  // namespace

int latents_import(const CellLayout& L, const int* cell_h, const int* cell_w, const float* z_where, const float* z_what, const float* z_depth,
                   const float* z_pres, float* nbox, float* rec, float* Za, void* Za16, hipStream_t s) {
    if (L.REC != L.A + 6 || L.ld_rec < L.REC) return SPAIR_ERR_SHAPE;      // the kernel writes rec column REC - 1 = A + 5 of every row
    const long long total = (long long)L.N * L.ld_rec;
    hipLaunchKernelGGL(k_latents_import, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, L, cell_h, cell_w, z_where, z_what, z_depth,
                       z_pres, nbox, rec, Za, reinterpret_cast<__bf16*>(Za16));
    SPAIR_CHECK_LAUNCH();
    return SPAIR_OK;
}

int render_layers(const RenderGeom& g, const float* S, int ld_s, int s16, int CH, const int* cidx, const int* cells, int K, const float* inv_den,
                  float* layers, float* layer_weight, hipStream_t s) {
    if (g.B <= 0 || g.HW <= 0 || g.I <= 0 || g.Iw <= 0 || g.P < 1 || K < 1 || ld_s < g.P * g.P * CH) return SPAIR_ERR_SHAPE;
    if (CH < 2 || CH > 4) return SPAIR_ERR_UNSUPPORTED;
    if ((long long)g.B * g.HW > 0x7fffffffLL) return SPAIR_ERR_UNSUPPORTED;
    const int blocks = g.B * ((g.Iw + RT - 1) / RT) * ((g.I + RT - 1) / RT);
#define SP_LAYERS_LAUNCH(S16_, C_)                                                                                                          \
    hipLaunchKernelGGL((k_render_layers<S16_, C_>), dim3(blocks), dim3(256), 0, s, S, ld_s, g.nbox, g.pres, g.depth, g.ld_pd, cidx, cells, K, \
                       inv_den, layers, layer_weight, g.B, g.HW, g.I, g.Iw, g.P, g.ac)
    if (s16) {
        if (CH == 2) SP_LAYERS_LAUNCH(true, 1); else if (CH == 3) SP_LAYERS_LAUNCH(true, 2); else SP_LAYERS_LAUNCH(true, 3);
    } else {
        if (CH == 2) SP_LAYERS_LAUNCH(false, 1); else if (CH == 3) SP_LAYERS_LAUNCH(false, 2); else SP_LAYERS_LAUNCH(false, 3);
    }
#undef SP_LAYERS_LAUNCH
    SPAIR_CHECK_LAUNCH();
    return SPAIR_OK;
}

// unit-level C ABI: rows r = (cidx ? cidx[k] : k) * B + b of sprites [N][ld_s], nbox [N][4], pres [N], depth [N]
extern "C" int spair_render_layers_rows(const void* sprites, int ld_s, int s16, int ch, const float* nbox, const float* pres, const float* depth,
                                        const int* cidx, const int* cells, int K, const float* inv_den, float* layers, float* layer_weight,
                                        int B, int HW, int I, int Iw, int P, int align_corners, void* stream) {
    if (!sprites || !nbox || !pres || !depth || !cells || !inv_den || !layers || !layer_weight) return SPAIR_ERR_SHAPE;
    return render_layers({nbox, pres, depth, 1, B, HW, I, P, align_corners, Iw}, reinterpret_cast<const float*>(sprites), ld_s, s16, ch, cidx,
                         cells, K, inv_den, layers, layer_weight, (hipStream_t)stream);
}
