// Scene composition from given latents (compose.hip): the inverse of the per-row -> NCHW export, and the renderer's composite kept per
// requested object (the layers of SPAIR.compose).
#pragma once
#include "cells.h"
#include "render.h"

// NCHW latent maps -> the workspace's per-cell rows r = cprime * B + b (cell_h / cell_w: cprime -> grid position): nbox [N][4] = z_where,
// rec columns 4 .. 4 + A (z_what), 4 + A (z_depth), REC - 1 (z_pres), the decoder's input rows Za (fp32, zero padded to ld_rec) and, where
// Za16 is not null, the same rounded to bf16.  rec columns 0 .. 3 (the box before its normalisation) are left alone: nothing after the
// per-cell chain reads them.
int latents_import(const CellLayout& L, const int* cell_h, const int* cell_w, const float* z_where, const float* z_what, const float* z_depth,
                   const float* z_pres, float* nbox, float* rec, float* Za, void* Za16, hipStream_t s);

// layers [B][K][C][I][Iw], layer_weight [B][K][I][Iw] of the cells `cells` [B][K] (row-major cell index; outside [0, HW): an all-zero
// layer) from sprites of CH = C + 1 elements per texel (alpha last; s16: fp16 elements, else fp32), the rows' nbox / presence / depth and the
// renderer forward's 1/D per pixel.  cidx: cell -> row block (rows cidx[k] * B + b) or null = identity.
int render_layers(const RenderGeom& g, const float* S, int ld_s, int s16, int CH, const int* cidx, const int* cells, int K, const float* inv_den,
                  float* layers, float* layer_weight, hipStream_t s);
