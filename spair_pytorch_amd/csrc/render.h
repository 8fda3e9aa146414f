// The renderer's host interface (K6, models.py:485-547).  A launcher runs its own kernel family only (SPAIR_ERR_UNSUPPORTED where its
// _supported predicate refuses); the caller chooses the family: render_plan for the training step, the unit entry points (render.hip) for
// the C ABI.  s16: fp16 (grey, alpha) sprites, ld_s in elements of that type; aux: B*C*I*Iw float2 (dBCE/dpre / D, pre); inv_den: B*I*Iw 1/D.
// The canvas is I rows x Iw columns; only the first generation (grey) and the generic-channel kernels take Iw != I.
#pragma once
#include "layout.h"

struct RenderGeom {           // the objects: nbox [N][4], pres / depth with row stride ld_pd, N = B * HW rows
    const float *nbox, *pres, *depth;
    int ld_pd, B, HW, I, P, ac;
    int Iw;                   // canvas width (I: its height)
};

int render_num_blocks(int B, int I, int Iw);   // forward workgroups = bce_partial entries (first generation / colour: 16 x 16 tiles of I x Iw)
int render_sprite_act(float* S, int ld, int N, int per, int CH, float obj_scale, float alpha_scale, float alpha_bias, hipStream_t s);
int render_prep_bytes(int B, int HW);

// render3.hip: per-object records (render_prep; it also refuses records that are not 16-byte aligned), the forward on the matrix cores
bool render_prep_supported(const RenderGeom& g);
bool render_fwd_mma_supported(const RenderGeom& g, const void* S16, int ld_s, const void* rec);
const void* render_rec_cull(const void* rec, int B, int HW);
const void* render_rec_bwd(const void* rec, int B, int HW);
int render_prep(const RenderGeom& g, void* rec, hipStream_t s);
int render_fwd_mma(const RenderGeom& g, const void* S16, int ld_s, const void* rec, const float* x, float* recon, float* aux, float* bce_partial,
                   float* inv_den, hipStream_t s);
// render2.hip: the tap forward k_render_fwd3; k_render_bwd2 (fp16 sprites, bf16 d-logits; rec: records or null)
bool render_fwd2_supported(const RenderGeom& g, const float* S, int ld_s, int s16);
bool render_bwd2_supported(const RenderGeom& g, const float* S, int ld_s, const float* dlogits, int ld_g);
int render_fwd2(const RenderGeom& g, const float* S, int ld_s, int s16, const float* x, float* recon, float* aux, float* bce_partial,
                float* inv_den, hipStream_t s);
int render_bwd2(const RenderGeom& g, const float* S, int ld_s, const void* rec, const float* aux, const float* gloss, float* dlogits, float* dnbox,
                float* dpres, float* ddepth, int ld_g, float obj_scale, float alpha_scale, hipStream_t s);
// render.hip: the first generation (g16: bf16 d-logits)
int render_fwd1(const RenderGeom& g, const float* S, int ld_s, int s16, const float* x, float* recon, float* aux, float* bce_partial,
                float* inv_den, hipStream_t s);
int render_bwd1(const RenderGeom& g, const float* S, int ld_s, int s16, const float* aux, const float* gloss, float* dlogits, float* dnbox,
                float* dpres, float* ddepth, int ld_g, float obj_scale, float alpha_scale, int g16, hipStream_t s);
// render_c.hip: C = 2 or 3 colour channels, fp32 sprites and d-logits [N][P*P][C+1]
int render_fwd_c(const RenderGeom& g, const float* S, int ld_s, int C, const float* x, float* recon, float* aux, float* bce_partial,
                 float* inv_den, hipStream_t s);
int render_bwd_c(const RenderGeom& g, const float* S, int ld_s, int C, const float* aux, const float* gloss, float* dlogits, float* dnbox,
                 float* dpres, float* ddepth, int ld_g, float obj_scale, float alpha_scale, hipStream_t s);

// The training step's renderer, decided once per call (render.hip)
enum RenderFamily { RENDER_MMA, RENDER_GEN2, RENDER_GEN1, RENDER_COLOUR };
struct RenderPlan {
    RenderFamily fwd, bwd;
    bool rec;                 // render_prep writes records before the decoder; k_render_bwd2 reads them, whichever forward ran
    bool s16, g16;            // fp16 sprites / bf16 d-logits (else fp32)
};
// 16-bit sprites and d-logits: the bf16 step's grey images with the MLP object decoder (the conv decoder and the colour kernels take fp32)
inline bool render_16bit(const SpairDims& d) { return d.dtype == SPAIR_BF16 && d.C == 1 && !d.obj_conv; }
RenderPlan render_plan(const SpairDims& d, const RenderGeom& g, int ld_s, const float* S, const void* rec, const float* dlogits);

// render_owner.hip: the scene parse's per-pixel owner map (arg-max of the composite's per-object coefficients; its own kernel family for
// every sprite format: s16 fp16 / fp32 elements, CH elements per texel with alpha last).  cidx: cell k (row-major) -> row block, or null
int render_owner(const RenderGeom& g, const float* S, int ld_s, int s16, int CH, const int* cidx, float threshold, int* owner,
                 float* owner_weight, float* coverage, int* area, hipStream_t s);
