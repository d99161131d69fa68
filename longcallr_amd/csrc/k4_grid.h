// k4_grid.h — launchers of the kernels that serve one region with all CUs, and of the chain-region kernels, for the host control in
// k4_phase.hip: k4_chain_wg / k4_chain_grid (k4_grid.hip), k4_stage_grid (k4_stage.hip), k4_gpost (k4_post.hip).
#pragma once
#include "k4_dev.h"

constexpr int K4_CHAIN_WG_THREADS = 1024;   // = K4_GRID_THREADS (below)

// one workgroup per chain region: regions desc[first .. first + n)
hipError_t k4_chain_launch_wg(const ChainDev& C, int first, int n, size_t dyn_lds, hipStream_t s);
// all CUs on the single region desc[which] (persistent launch with grid barriers; C.ctl is reset here)
hipError_t k4_chain_launch_grid(const ChainDev& C, int which, size_t dyn_lds, hipStream_t s);
// k4_chain_wg's static stage rows (sixteen waves x four rows of 65 doubles): racc of the row-balanced cross_optimize and the scratch of
// the LDS pair table between block flips; SNPs whose constants it keeps in LDS
constexpr int K4_CHAIN_STAGE_BYTES = (K4_CHAIN_WG_THREADS / 64) * 4 * 65 * 8;
constexpr int K4_CHAIN_SCN = 256;
// dynamic LDS the device-coherent perturbation rounds may use (sigma bit vector + delta / eta / het-delta bytes of the region)
constexpr int K4_GRID_FAST_LDS_MAX = 96 * 1024;
inline size_t k4_grid_fast_lds(int64_t R, int64_t S) { return (size_t)(8 * ((R + 63) / 64) + 3 * S + 64); }
// the batched rounds (k4_grid_batch.h): spread masks of every SNP + team slots + set-up histogram
constexpr int K4_GRID_BATCH_MAX_WG = 512;
constexpr int K4_GRID_BATCH_CTL_BYTES = 128 + 2048 + 128 + K4_GRID_BATCH_MAX_WG * 128;
inline size_t k4_grid_batch_lds(int64_t S) { return (size_t)(12 * (S + 2) + 24 * 1024); }
// threads per workgroup / workgroups of a grid launch (co-resident by construction); 0 = no device
constexpr int K4_GRID_THREADS = 1024;
int k4_grid_blocks();
// k4_stage_grid (k4_stage.hip): one large region with all CUs; blk_tot: 3 * k4_grid_blocks() + 1 int32 of scratch
hipError_t k4_stage_launch_grid(const StageIn& in, const StageOut& out, const PhaseLutDev& lut, int g, GridCtl* ctl, int32_t* blk_tot, hipStream_t s);
// k4_gpost (k4_post.hip): post-phase steps for one large region with all CUs
hipError_t k4_post_launch_grid(const PostIn& post_in, const PostScratch& ps, int g, const PostLut& lut, hipStream_t s);
// hipFuncSetAttribute(MaxDynamicSharedMemorySize) once per (kernel slot 0..7, device) (k4_grid.hip)
hipError_t k4_set_dyn_lds_once(const void* fn, int bytes, int slot);
