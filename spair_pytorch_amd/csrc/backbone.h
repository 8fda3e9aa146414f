// The backbone's patch-resident kernels of the bf16 step: 128 -> 128 channel 4x4 / stride-2 convolutions on bf16 NHWC activations.  A launcher
// returns SPAIR_ERR_UNSUPPORTED exactly where its _supported predicate refuses; the step plan (engine.hip, plan_step) asks the predicates and
// the launch code never falls back.
#pragma once
#include "common.h"
#include "spair_hip.h"

// conv_s2.hip: forward (+ bias + relu), weights in tap-parity K order (gemm.h, GemmNT::ktab); mask: optional sign bits of the output
// [B*Hout*Hout][16] bytes (the next layer's data-gradient gate)
bool conv_s2k4_patch_fwd16_supported(int B, int Hin, int Hout, int cin, int cout, int k, int s_);
int conv_s2k4_patch_fwd16(const void* in, const void* wf, const float* bias, void* out, int B, int Hin, int Hout, int cin, int cout, int k, int s_,
                          hipStream_t s, void* mask = nullptr);
// conv_s2_dgrad.hip: data gradient (all 4 output-parity classes per workgroup), ReLU gate of the layer below, optionally with the stem's weight
// gradient fused (stem_part != nullptr: nothing is stored to `out`; _stem_supported); gate_bits != nullptr: the gate as sign bits, one byte
// per (pixel, 8 channels) -- what the stem kernel (misc.hip) or the patch forward leaves -- instead of the activation itself
bool conv_s2k4_patch_dgrad16_supported(int B, int Ho, int hin, int cin, int cout, int k, int s_);
// the tiling of the 128 -> 128 channel data gradient alone (tiles of 128 class pixels; tpi: tiles per image, 0 = whole-batch tiles), or false:
// the part of the launcher's geometry check that needs no device (the persistent grid = min(tiles, CUs) is chosen at the launch)
bool conv_s2k4_patch_dgrad16_tiling(int B, int Ho, int& tiles, int& tpi);
bool conv_s2k4_patch_dgrad16_stem_supported(int B, int Ho, int hin, int cin, int cout, int k, int s_, int stem_hin, int stem_s, long long stem_part_cap);
int conv_s2k4_patch_dgrad16(const void* dout, const void* const* wd, const void* gate, void* out, int B, int Ho, int hin, int cin, int cout, int k,
                            int s_, const float* stem_xp, int stem_hin, int stem_s, float* stem_part, long long stem_part_cap, float* stem_dw,
                            float* stem_db, hipStream_t s, const void* gate_bits = nullptr);

// The training step's plan names (engine.hip, plan_step; reported by spair_step_plan).  A backbone layer's forward or data-gradient kernel: one
// implicit-GEMM launch in the step's dtype (a strided data gradient: all output-parity classes in it), the patch-resident kernel, one launch per
// output-parity class, or the fused trailing 1x1 stack (pointwise.hip)
enum ConvKernel { CONV_GEMM = SPAIR_CONV_GEMM, CONV_PATCH = SPAIR_CONV_PATCH, CONV_PER_CLASS = SPAIR_CONV_PER_CLASS, CONV_PW_STACK = SPAIR_CONV_PW_STACK };
// where the stem's weight gradient is taken: fused into conv_1's patch-resident or implicit-GEMM data gradient (d act0 never reaches HBM;
// SpairStep.flags bit 3 turns both off), the grey-scale 4x4 stem's own kernel, or the generic TN GEMM
enum StemWgrad { STEM_PATCH = SPAIR_STEM_PATCH, STEM_GEMM = SPAIR_STEM_GEMM, STEM_WGRAD16 = SPAIR_STEM_WGRAD16, STEM_GENERIC = SPAIR_STEM_GENERIC };
