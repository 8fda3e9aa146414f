// Adjoints of the step's three map outputs folded into the hand-written backward (SpairStepIO.grad_recon, grad_z_where, grad_z_pres).
//
// The reference returns all three as live autograd tensors (models.py:35-131), so a user term on any of them trains through the
// whole model.  Every engine path shares the entry points these kernels feed, so they are the whole feature:
//  * recon = clamp(pre, 0, 1): the renderer backward consumes aux[pixel] = (dBCE/dpre / D, pre) scaled by *grad_loss.  The external
//    term adds g_recon * [0 <= pre <= 1] / D (torch's inclusive clamp mask, the one the BCE term uses).  It is folded into a SEPARATE
//    copy aux_ext = (gloss * aux.x + g_recon * mask * inv_den, aux.y) and the unchanged renderer backward then runs on aux_ext with a
//    loss gradient of 1: the forward's aux stays untouched, so a second backward through the same forward (retain_graph) sees it again.
//  * z_where / z_pres are the renderer's nbox / presence inputs: their adjoints are added to the per-row renderer gradients
//    g_nbox_r[r][4] / g_pres_r[r] after the renderer backward wrote them and before the per-cell backward reads them.  Row r is
//    (cell position cp = r / B, sample b = r % B) and cp -> (h, w) through the workspace's cell tables -- the mapping the forward's
//    z_where / z_pres export uses on both the per-wavefront launches and the fused chain, for every N_LOOKBACK.
// Plain elementwise kernels: one element (or row) per thread, no atomics, so the step stays bit-for-bit repeatable.
#include "cells.h"

__global__ __launch_bounds__(256) void k_recon_fold(const float2* __restrict__ aux, const float* __restrict__ gloss,
                                                    const float* __restrict__ grad_recon, const float* __restrict__ inv_den,
                                                    float2* __restrict__ aux_ext, float* __restrict__ one, long long n, int C, long long npix) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i == 0) *one = 1.f;
    if (i >= n) return;
    const float gl = *gloss;
    const float2 av = aux[i];                                  // index ((b * C + c) * I + y) * Iw + x, the recon layout
    const long long per = (long long)C * npix, b = i / per, pix = (i - b * per) % npix;
    const float pre = av.y;
    const float ext = (pre >= 0.f && pre <= 1.f) ? grad_recon[i] * inv_den[b * npix + pix] : 0.f;
    aux_ext[i] = make_float2(gl * av.x + ext, av.y);
}

__global__ __launch_bounds__(256) void k_rows_fold(const int* __restrict__ cell_h, const int* __restrict__ cell_w, int B, int G, int Gw,
                                                   const float* __restrict__ g_z_where, const float* __restrict__ g_z_pres,
                                                   float* __restrict__ g_nbox_r, float* __restrict__ g_pres_r) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= B * G * Gw) return;
    const int cp = r / B, b = r - cp * B;
    const int hw = cell_h[cp] * Gw + cell_w[cp];
    if (g_z_where) {
#pragma unroll
        for (int k = 0; k < 4; ++k) g_nbox_r[(size_t)r * 4 + k] += g_z_where[((size_t)b * 4 + k) * G * Gw + hw];
    }
    if (g_z_pres) g_pres_r[r] += g_z_pres[(size_t)b * G * Gw + hw];
}

// aux / aux_ext: n = B*C*I*Iw float2; grad_recon [B][C][I][Iw]; inv_den [B][I][Iw]; `one` receives 1.0f (the renderer's loss gradient)
int outgrad_recon_fold(const float* aux, const float* gloss, const float* grad_recon, const float* inv_den, float* aux_ext, float* one, int B,
                       int C, int I, int Iw, hipStream_t s) {
    const long long npix = (long long)I * Iw, n = (long long)B * C * npix;
    if (n <= 0) return SPAIR_ERR_SHAPE;
    hipLaunchKernelGGL(k_recon_fold, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, reinterpret_cast<const float2*>(aux), gloss,
                       grad_recon, inv_den, reinterpret_cast<float2*>(aux_ext), one, n, C, npix);
    SPAIR_CHECK_LAUNCH();
    return SPAIR_OK;
}

// g_z_where [B][4][G][Gw] and g_z_pres [B][1][G][Gw] (either may be null) into the renderer's per-row gradients
int outgrad_rows_fold(const int* cell_h, const int* cell_w, int B, int G, int Gw, const float* g_z_where, const float* g_z_pres, float* g_nbox_r,
                      float* g_pres_r, hipStream_t s) {
    if (!g_z_where && !g_z_pres) return SPAIR_OK;
    const int n = B * G * Gw;
    hipLaunchKernelGGL(k_rows_fold, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, cell_h, cell_w, B, G, Gw, g_z_where, g_z_pres, g_nbox_r,
                       g_pres_r);
    SPAIR_CHECK_LAUNCH();
    return SPAIR_OK;
}
