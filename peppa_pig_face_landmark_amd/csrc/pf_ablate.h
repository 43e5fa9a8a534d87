// The ablation flavour of the library: PF_ABLATE, the PEPPA_DBG bit mask and the cycle-counter buffer, for kernels and host alike.
//
// `python -m peppa_pig_face_landmark_amd.build --ablate` compiles the same sources with -DPF_ABLATE=1 into libpeppa_hip_ablate.so
// for tools/ab_env.py; pf_create reads PEPPA_DBG there into pf_handle::dbg and the launchers copy it into the `dbg` field of the
// kernels' argument structs.  In the production library pf_dbg() and host_dbg() (engine.cpp) are the constant 0: every ablation
// branch folds away, and no environment variable can make a kernel skip work or switch the range guard off.
//
// The bits, in three groups:
//   skip     a kernel leaves work out to show what paces it: results are WRONG
//   select   the host launches another instance or takes another path: results are right
//   account  cycle counters are collected and printed at pf_destroy: results are right
// The values are what the recorded tables (profiles/r02_*ablations.md and later) and the tools/ scripts pass, so they stay as they
// are, and ONE VALUE MEANS DIFFERENT THINGS in different kernels: one name per meaning below, same value.
//
//   value   group    read by                                                              effect
//   1       skip     k_halo.h, k_sepup_patch.h                                            weights fetched for the first K step only
//           skip     k_sepup.h sepup_pipe_kernel (w_issue, either role)                   no weight requests after the prologue's
//           skip     k_mbx.h                                                              no weight / constant DMA after tile 0's round
//   2       skip     k_sepup.h producers                                                  no patch / filter / skip-chunk requests (dma_issue)
//           skip     k_mbx.h depthwise                                                    no depthwise taps
//   4       skip     k_sepup.h producers                                                  patch not read from LDS (zeros are filtered)
//           skip     k_mbx.h expand, project                                              no MFMAs
//   8       skip     k_sepup.h consumers                                                  no MFMAs
//   16      skip     k_conv_split.h, k_halo.h, k_chain.h                                  no MFMAs
//           skip     k_sepup.h consumers (store_vec), k_mbx.h (mode 3 map, projection)    no output stores
//   32      skip     k_conv_gemm.h epilogue, k_expdw.h, k_chain.h                         no output stores
//   64      skip     k_halo.h, k_sepup_patch.h                                            input patch staged for the first channel chunk only
//           account  k_sepup.h sepup_pipe_kernel, k_mbx.h; launch_sepup, launch_mbx       per-role / per-wave cycle totals
//   128     skip     k_halo.h                                                             no per-tap barrier
//   256     skip     k_conv_split.h                                                       operands (pixels AND weights) of the first K step only
//           skip     k_sepup_patch.h                                                      one patch row of three
//   512     skip     k_conv_split.h                                                       no split / LDS store of the pixel operand
//   1024    skip     k_expdw.h (depthwise epilogue of the 16 x 16 expdw instances)        no depthwise taps
//           select   launch_conv (LDS-resident 3x3 family)                                no 256-pixel tiles of the narrow halo instances
//   2048    select   launch_conv                                                          hero conv -> halo kernel
//           select   launch_sepup                                                         pipelined kernel -> patch kernel
//   4096    account  launch_detunit, launch_hrb (k_det.h, k_hrb.h test a.prof, not the bit) per-phase cycle totals
//   16384   select   launch_conv                                                          conv3x3_hero_kernel<4, false>, an A/B instance
//   32768   select   nothing but pf_create's guard mask                                   range guard off, everything else as in production
//   524288  select   launch_conv (score head)                                             pw_head_kernel -> conv_gemm_split_kernel
//
// Collisions to know before a run: 64 for sepup's or mbx's cycle counters also corrupts every halo and patch conv of the run;
// 1024 for the narrow halo tiles also takes the depthwise taps out of every 16 x 16 expdw launch; 1, 2, 4, 16 and 256 each skip
// something in every kernel listed against them, and 16 is MFMAs in one family and stores in another.
#pragma once
#include <hip/hip_runtime.h>

#ifndef PF_ABLATE
#define PF_ABLATE 0
#endif
template <typename Args> __device__ __forceinline__ int pf_dbg(const Args& a) { return PF_ABLATE ? a.dbg : 0; }

// ---- skip work: results are wrong ---------------------------------------------------------------------------------------------------
constexpr int PF_ABL_W_FIRST_K = 1;             // k_halo.h, k_sepup_patch.h
constexpr int PF_ABL_SEPUP_NO_W_DMA = 1;        // k_sepup.h
constexpr int PF_ABL_MBX_DMA_FIRST_TILE = 1;    // k_mbx.h
constexpr int PF_ABL_SEPUP_NO_P_DMA = 2;        // k_sepup.h
constexpr int PF_ABL_MBX_NO_DW_TAPS = 2;        // k_mbx.h
constexpr int PF_ABL_SEPUP_NO_PATCH_READS = 4;  // k_sepup.h
constexpr int PF_ABL_MBX_NO_MFMA = 4;           // k_mbx.h
constexpr int PF_ABL_SEPUP_NO_MFMA = 8;         // k_sepup.h
constexpr int PF_ABL_NO_MFMA = 16;              // k_conv_split.h, k_halo.h, k_chain.h
constexpr int PF_ABL_SEPUP_NO_STORE = 16;       // k_sepup.h
constexpr int PF_ABL_MBX_NO_STORE = 16;         // k_mbx.h
constexpr int PF_ABL_NO_STORE = 32;             // k_conv_gemm.h, k_expdw.h, k_chain.h
constexpr int PF_ABL_PATCH_FIRST_CHUNK = 64;    // k_halo.h, k_sepup_patch.h
constexpr int PF_ABL_HALO_NO_TAP_BARRIER = 128; // k_halo.h
constexpr int PF_ABL_OPERANDS_FIRST_K = 256;    // k_conv_split.h
constexpr int PF_ABL_PATCH_ONE_ROW = 256;       // k_sepup_patch.h
constexpr int PF_ABL_NO_SPLIT_STORE = 512;      // k_conv_split.h
constexpr int PF_ABL_EXPDW_NO_DW_TAPS = 1024;   // k_expdw.h
// ---- select: another instance or path, results are right -------------------------------------------------------------------------
constexpr int PF_SEL_HALO_TILES_128 = 1024;     // launch_conv
constexpr int PF_SEL_HERO_TO_HALO = 2048;       // launch_conv
constexpr int PF_SEL_SEPUP_TO_PATCH = 2048;     // launch_sepup
constexpr int PF_SEL_HERO_AB = 16384;           // launch_conv
constexpr int PF_SEL_GUARD_OFF_ONLY = 32768;    // pf_create, through PF_DBG_GUARD_OFF_MASK alone
constexpr int PF_SEL_NO_PW_HEAD = 524288;       // launch_conv
// ---- account: cycle counters, results are right ----------------------------------------------------------------------------------
constexpr int PF_ACC_CYCLES = 64;               // k_sepup.h, k_mbx.h, launch_sepup, launch_mbx
constexpr int PF_ACC_DET_CYCLES = 4096;         // launch_detunit, launch_hrb

// pf_create switches the f32s range guard off when PEPPA_DBG has a bit of this mask: every skip bit lies in it (ablated kernels
// compute garbage), and so do the select / account bits below 65536, whose runs would pass the guard -- 64 and 1024 share their
// value with a skip bit, 2048, 4096 and 16384 are merely inside the mask, and 32768 exists to switch the guard off and nothing
// else.  Of today's bits only 524288 lies outside: results right, guard on.
constexpr int PF_DBG_GUARD_OFF_MASK = 0xffff;

// ---- cycle counters (pf_handle::d_dbg): words of 64 bits, entry e of a region at base + e * words -----------------------------------
struct PfCycleRegion {
    int base, words, entries;
    constexpr int at(int e) const { return base + e * words; }
};
constexpr PfCycleRegion PF_CYC_SEPUP = {0, 16, 2};      // entry: BN 128 / 256.  k_sepup.h: [0] producer work, [1] producer wait, [2] producer
                                                        // waves, [3] their K steps, [4 .. 7] consumer dma / mfma / epilogue / wait, [8] consumer waves, [9] producer dma
constexpr PfCycleRegion PF_CYC_DETUNIT = {64, 8, 6};    // entry: (C 32 / 64 / 128) + 3 * (stride - 1).  k_det.h: four phases, [4] workgroups
constexpr PfCycleRegion PF_CYC_HRB = {144, 4, 2};       // entry: CIN 64 / 256.  k_hrb.h: conv1 / conv2 / conv3, [3] workgroups
constexpr PfCycleRegion PF_CYC_MBX = {160, 8, 16};      // entry: shape * 4 + mode.  k_mbx.h: seven phases, [7] waves
constexpr int PF_CYC_WORDS = 64 * 16;                   // size of the buffer
static_assert(PF_CYC_MBX.base + PF_CYC_MBX.words * PF_CYC_MBX.entries <= PF_CYC_WORDS, "the regions fit the buffer");
