// SPAIR.evaluate: the loss's terms per image, per cell and per pixel, from stored operands (evaluate.hip).
#pragma once
#include "cells.h"

#define EVAL_MAX_HW 1024       // the library's grid limit (loss.hip: KL_MAXBINS - 1)
#define EVAL_MAX_SLICES 256    // workgroups one sample is split over
#define EVAL_NPART 8           // floats per workgroup partial: BCE, the six Gaussian KLs, the presence KL

// Per-row operands: element (r, col) of an array is p[r * ld + col]; row r = (cidx ? cidx[k] : k) * B + b for cell k = h * Gw + w.
// mu_box / sd_box hold the four columns cy, cx, height, width; mu_attr / sd_attr the A attribute columns; the others one column.
struct EvalRows {
    const float *z_pres, *p_z, *mu_box, *sd_box, *mu_attr, *sd_attr, *mu_depth, *sd_depth;
    int ld_z, ld_pz, ld_mu_box, ld_sd_box, ld_mu_attr, ld_sd_attr, ld_mu_depth, ld_sd_depth;
    const int* cidx;
    float prior_mean[6], prior_std[6];      // cy, cx, height, width, attr, depth
};

// workgroups per sample (1 .. EVAL_MAX_SLICES): a function of the shape alone, so the scratch size and the summation order are too
int eval_slices(int B, int HW, long long npix);
// floats of scratch a call needs: B * eval_slices * EVAL_NPART
long long eval_scratch_floats(int B, int HW, long long npix);
// terms [B][9], kl_map [B][7][HW] or NULL, bce_map [B][I*Iw] or NULL; every argument is checked before the first launch (SPAIR_ERR_SHAPE)
int eval_sample_terms(const EvalRows& R, int B, int HW, int A, int C, int I, int Iw, float beta, const float* recon, const float* x,
                      float* terms, float* kl_map, float* bce_map, float* scratch, int accumulate, float scale, hipStream_t s);
