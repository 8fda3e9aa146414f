// SPAIR.generate: latents drawn from the model's own prior (prior.hip).
#pragma once
#include "cells.h"

#define PRIOR_MAX_HW 1024      // HW + 1 count bins <= 1025, the library's limit (loss.hip: KL_MAXBINS)

// z_pres / p_z [B][HW] (row-major cells), n_present [B] from u [B][HW]: the sequential count prior started from the geometric distribution
// of `prior_prob`, or, for a sample with count[b] (count != NULL), from the one-hot distribution at clamp(count[b], 0, HW)
int prior_presence(const float* u, int B, int HW, float prior_prob, const int* count, float* z_pres, float* p_z, int* n_present,
                   hipStream_t s);
// the Gaussian latents pushed through the forward's transforms (cell_math.h): NCHW eps maps in, NCHW z_where / z_what / z_depth out
int prior_gauss_maps(const CellHyper& H, int B, int A, int G, int Gw, const float* eps_box, const float* eps_attr, const float* eps_depth,
                     float* z_where, float* z_what, float* z_depth, hipStream_t s);
