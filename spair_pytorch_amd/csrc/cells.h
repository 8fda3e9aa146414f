// Buffers and hyper-parameters shared by the per-cell kernels (cells.hip, stn.hip, render.hip,
// loss.hip, outgrad.hip) and the host orchestration (engine.hip), and the launchers engine.hip calls in them.
#pragma once
#include "layout.h"

// per-row statistics kept for the backward pass / KL
#define SP_LDSTAT 16
#define ST_MU_BOX 0    // 4: cy, cx, height, width (post-freeze)
#define ST_SD_BOX 4    // 4
#define ST_MU_DEPTH 8
#define ST_SD_DEPTH 9
#define ST_PZ 10       // count-prior probability p(z_pres=1 | counts so far)

struct CellHyper {
    float wheel;              // LATENT_VAR_TRAINING_WHEEL (0 or 1 with the reference config)
    float kl_scale;           // 1 / (B * world_size)
    float img;                // image side I (float)
    float anchor;             // ANCHORBOX_SHAPE[0]
    float cell_over_img;      // pixels_per_cell / I  (computed in double, rounded once: models.py:373)
    float max_yx, min_yx, max_hw, min_hw;
    float prior_mean[6], prior_std[6];   // cy, cx, height, width, attr, depth
    float count_prior_prob;   // sigmoid(log(v+1e-6)), models.py:186-188
    float range_yx, range_hw; // max - min of the two box ranges (fp32 differences, formed on the host: the chain kernels take them as scalar
                              // operands -- formed in the kernel the compiler hoists them into vector registers the forward chain does not have)
    // the width axis: img and cell_over_img above are the height axis (image rows I); the same two for the image width Iw (= them when square)
    float img_w, cell_over_w;
};

struct CellBufs {
    // tables (device)
    const int *cell_h, *cell_w, *cidx, *nbr, *cons, *diag_start;
    // inputs
    const float* feat; int ld_feat;
    const float* edge;
    const float *eps_box, *eps_attr, *eps_depth, *u_pres;   // NCHW maps [B,{4,A,1,1},G,Gw]
    const float* gloss;                                     // device scalar dL/dloss
    // forward activations (row-major, row r = cprime*B + b)
    float *Xb, *Hb1, *Hb2, *Ob;
    float *glimpse, *He1, *He2, *Oe;
    float *Xz, *Hz1, *Hz2, *Oz;
    float *Xo, *Ho1, *Ho2, *Oo;
    float *rec, *sd_attr, *nbox, *stat;
    float* Za;                                              // attr rows for the decoder [N, ld_rec], zero padded
    void *Za16, *dfeat16;                                   // fused chain (bf16 step): the same two tensors written directly as bf16
    unsigned long long* mbits;                              // fused chain only: relu sign bits of the 8 hidden layers, [B][3G-2][66 tiles][4] wave ballots
    unsigned int* gxy;                                      // fused chain only: per glimpse element (d val/d gx, d val/d gy) as fp16x2 [N, ld_gl]
    float *z_where, *z_pres;                                // NCHW outputs
    // backward
    float *dXb, *dHb1, *dHb2, *dOb;
    float *dGl, *dHe1, *dHe2, *dOe;
    float *dXz, *dHz1, *dHz2, *dOz;
    float *dXo, *dHo1, *dHo2, *dOo;
    float *grec, *g_nbox_stn;
    float *g_nbox_r, *g_pres_r, *g_depth_r, *g_attr_r;      // from the renderer / decoder
    float* dfeat;
};

int cells_init_tables(int G, int Gw, int LB, int* cell_h, int* cell_w, int* cidx, int* nbr, int* cons, int* diag_start, hipStream_t s);
int cells_ctx_gather(const CellLayout& L, const CellBufs& P, int r0, int R, hipStream_t s);
int cells_box_sample(const CellLayout& L, const CellBufs& P, const CellHyper& H, int r0, int R, hipStream_t s);
int cells_attr_sample(const CellLayout& L, const CellBufs& P, int r0, int R, hipStream_t s);
int cells_depth_sample(const CellLayout& L, const CellBufs& P, const CellHyper& H, int r0, int R, hipStream_t s);
int cells_pres_sample(const CellLayout& L, const CellBufs& P, const CellHyper& H, int r0, int R, hipStream_t s);
int cells_bwd_pres(const CellLayout& L, const CellBufs& P, const CellHyper& H, int r0, int R, hipStream_t s);
int cells_bwd_depth(const CellLayout& L, const CellBufs& P, const CellHyper& H, int r0, int R, hipStream_t s);
int cells_bwd_attr(const CellLayout& L, const CellBufs& P, const CellHyper& H, int r0, int R, hipStream_t s);
int cells_bwd_box(const CellLayout& L, const CellBufs& P, const CellHyper& H, int r0, int R, hipStream_t s);
int cells_dfeat_edge(const CellLayout& L, const CellBufs& P, float* gedge, hipStream_t s);

// stn.hip (rows r0 .. r0+R-1, row r reads image r % B), outgrad.hip, loss.hip
// (images [B,C,Ih,Iw])
int stn_glimpse_fwd(const float* x, const float* nbox, int B, float* out, int ld, int r0, int R, int C, int Ih, int Iw, int P, int ac, int px16,
                    hipStream_t s);
int stn_glimpse_bwd(const float* x, const float* nbox, int B, const float* dgl, int ld, float* dnbox, int r0, int R, int C, int Ih, int Iw, int P,
                    int ac, int px16, hipStream_t s);
int outgrad_recon_fold(const float* aux, const float* gloss, const float* grad_recon, const float* inv_den, float* aux_ext, float* one, int B,
                       int C, int Ih, int Iw, hipStream_t s);
int outgrad_rows_fold(const int* cell_h, const int* cell_w, int B, int G, int Gw, const float* g_z_where, const float* g_z_pres, float* g_nbox_r,
                      float* g_pres_r, hipStream_t s);
int loss_count_kl(const CellLayout& L, const CellBufs& P, float prior_prob, float* klp, hipStream_t s);
int loss_gauss_kl_blocks(const CellLayout& L);
int loss_gauss_kl(const CellLayout& L, const CellBufs& P, const CellHyper& H, float* partial, hipStream_t s);
int loss_finalize(const float* bce_partial, int n_bce, const float* kl_partial, int n_kl, const float* klp, int B, float kl_scale, float beta, float* loss_out, const int* failed, int* status, int* status_host, int train, hipStream_t s);
