// Host launchers of the kernel files, declared once: every .hip file that defines one and every caller includes this header, so a changed
// signature fails to compile instead of failing to link.
#pragma once
#include "sf_device.h"

#include <algorithm>

namespace sf {
// ---- the tiled conv kernels (conv_igemm.hip) and their tile shapes: the ONE place that says which instantiations exist.  dispatch.hip
// (tiled_plan) picks a row, conv_igemm.hip maps (row, epilogue) to the instantiation, the profiler reports the row's key
// (_lib.py KERNEL_NAMES[key * 8 + epilogue]).
enum TileStaging { TILE_STAGED, TILE_DMA, TILE_DIRECT };      // conv_igemm_kernel (registers -> LDS) / conv_glds_kernel (LDS-DMA) / conv_direct_kernel (no LDS)
enum TileId {
  TILE_S16x64K4, TILE_L64x64, TILE_LN64x128, TILE_DIRECT16, TILE_SPLIT64x64, TILE_L128x128,
  TILE_DMA128x128, TILE_DMA64x64, TILE_DMA64x128, TILE_DMA64x256, TILE_DMA64x128W4, TILE_DMA32x128, TILE_DMA32x32, TILE_DMA_LN64x128, TILE_DMA_LN128x64, TILE_DMA_SPLIT64x64,
  TILE_COUNT, TILE_NONE = -1
};
constexpr int EPI_COUNT = 5;
constexpr unsigned E_AFFINE = 1u << EPI_AFFINE, E_BLEND = 1u << EPI_BLEND, E_LNG = 1u << EPI_LNG, E_TRUST = 1u << EPI_TRUST, E_SAMPLE = 1u << EPI_SAMPLE;
constexpr unsigned E_PLAIN = E_AFFINE | E_BLEND, E_LN = E_LNG | E_TRUST, E_ALL = E_PLAIN | E_LN | E_SAMPLE;
constexpr unsigned E_SCALE = E_AFFINE | E_SAMPLE;      // the epilogues of every SE-scaled (SCALE) instantiation of the LDS-DMA kernel
struct TileRow {
  TileStaging staging;
  int MT, NT, WM, WN, KS;      // a wave computes 16 MT output channels x 16 NT pixels, a workgroup WM x WN waves (x KS K-groups, staged kernel only);
                               // the direct kernel takes its MT (1, 2, 4) and KS (1..8) at run time: TiledPlan::mt / ks
  unsigned epis;               // epilogues instantiated for the row (E_* bits)
  // LDS-DMA rows: the row whose SCALE instantiation (epilogues E_SCALE) runs a launch with an SE input scale or the sampling epilogue — the
  // row itself where it has one, the 64 x 64 tile for the larger tiles, none for the LayerNorm tiles.  The staged and the direct kernel apply the
  // scale in their one instantiation
  TileId scaled_as;
  int key;                     // the profiler key the row reports — ALSO where another row's instantiation runs ("reported as")
};
constexpr TileRow TILES[TILE_COUNT] = {
    // "S": small pixel counts (BEV latent 50x50): 16 px x 64 cout per workgroup, 4-way in-workgroup split-K
    /* TILE_S16x64K4      */ {TILE_STAGED, 4, 1, 1, 1, 4, E_ALL, TILE_NONE, 0},
    // "L": large pixel counts (200x200 head): 2x2 waves of 32x32
    /* TILE_L64x64        */ {TILE_STAGED, 2, 2, 2, 2, 1, E_PLAIN | E_SAMPLE, TILE_NONE, 1},
    // LN-capable large tile: 4 waves x (64 cout x 32 px)
    /* TILE_LN64x128      */ {TILE_STAGED, 4, 2, 1, 4, 1, E_LN, TILE_NONE, 2},
    /* TILE_DIRECT16      */ {TILE_DIRECT, 0, 1, 1, 1, 0, E_ALL, TILE_NONE, 3},
    // "T": 4 waves x (64 cout x 16 px) = 64x64 tile, every epilogue; used with cross-WG split-K
    /* TILE_SPLIT64x64    */ {TILE_STAGED, 4, 1, 1, 4, 1, E_ALL, TILE_NONE, 4},
    // 128 x 128, 8 waves (2x4) of 64x32
    /* TILE_L128x128      */ {TILE_STAGED, 4, 2, 2, 4, 1, E_PLAIN, TILE_NONE, 9},
    // 128 cout x 128 px, 8 waves of 64x32.  SE-scaled launches run the 64 x 64 tile and are REPORTED AS key 10
    /* TILE_DMA128x128    */ {TILE_DMA, 4, 2, 2, 4, 1, E_PLAIN, TILE_DMA64x64, 10},
    // 64 cout x 64 px, 4 waves of 32x32
    /* TILE_DMA64x64      */ {TILE_DMA, 2, 2, 2, 2, 1, E_PLAIN, TILE_DMA64x64, 11},
    // 64 cout x 128 px, 8 waves of 32x32.  SE-scaled launches run the 64 x 64 tile and are REPORTED AS key 12
    /* TILE_DMA64x128     */ {TILE_DMA, 2, 2, 2, 4, 1, E_PLAIN, TILE_DMA64x64, 12},
    // 64 cout x 256 px, 8 waves of 32x64 (64-channel layers at large P: the staged bytes per FLOP of the 128 x 128 tile).  SE-scaled: as above
    /* TILE_DMA64x256     */ {TILE_DMA, 2, 4, 2, 4, 1, E_PLAIN, TILE_DMA64x64, 12},
    // 64 cout x 128 px, 4 waves of 64x32: an experiment's tile, reached by SF_NARROW=7 alone (dispatch.hip: narrow_tile).  REPORTED AS key 11 ("dma64x64")
    /* TILE_DMA64x128W4   */ {TILE_DMA, 4, 2, 1, 4, 1, E_PLAIN, TILE_DMA64x64, 11},
    // 32 cout x 128 px, 4 waves of 16x64 (narrow layers: 16- / 32-channel sparse stages).  REPORTED AS key 11 ("dma64x64")
    /* TILE_DMA32x128     */ {TILE_DMA, 1, 4, 2, 2, 1, E_PLAIN, TILE_DMA64x64, 11},
    // small pixel counts (one 50x50 latent): 32 cout x 32 px, 4 waves of 16x16.  REPORTED AS key 11 ("dma64x64")
    /* TILE_DMA32x32      */ {TILE_DMA, 1, 1, 2, 2, 1, E_PLAIN, TILE_DMA32x32, 11},
    // LayerNorm epilogues: one wave holds all (<= 64) output channels of its pixels; 64 cout x 128 px, 4 waves
    /* TILE_DMA_LN64x128  */ {TILE_DMA, 4, 2, 1, 4, 1, E_LN, TILE_NONE, 13},
    // LayerNorm epilogues over 65..128 output channels (hidden sizes no shipped config uses): 128 cout x 64 px, 4 waves of 128x16
    /* TILE_DMA_LN128x64  */ {TILE_DMA, 8, 1, 1, 4, 1, E_LN, TILE_NONE, 5},
    // cross-workgroup split-K launches: 64 cout x 64 px, 4 waves of 64x16 (all channels of a pixel in one wave)
    /* TILE_DMA_SPLIT64x64 */ {TILE_DMA, 4, 1, 1, 4, 1, E_PLAIN | E_LN, TILE_DMA_SPLIT64x64, 15},
};
// one launcher entry per staging; hipErrorInvalidValue where the table has no instantiation for (tile, epilogue)
hipError_t launch_conv(const ConvLaunch& L, int epi, TileId tile, hipStream_t stream);
hipError_t launch_conv_direct(const ConvLaunch& L, int epi, int mt, int ks, hipStream_t stream);      // TILE_DIRECT16; mt: 16-row cout tiles per wave (1, 2, 4); ks: K-groups per workgroup (1..8)
hipError_t launch_conv_glds(const ConvLaunch& L, int epi, TileId tile, hipStream_t stream);
hipError_t launch_conv_glds_producer(const ConvLaunch& L, hipStream_t stream);      // TILE_DMA128x128, AFFINE: the first input channels computed in the workgroup (conv_igemm.hip: PROD)
hipError_t set_stamp_buffer(unsigned long long* p);
int glds_occupancy(int which);

// ---- launcher boilerplate shared by conv_igemm.hip, conv_sp.hip and conv_wino.hip (host only)
// The dynamic-LDS limit of kernel Kern, raised to `bytes` on the first call per device (a process may touch more than one GPU).  One process
// per GPU and one launching thread per device are the documented use (include/sfnative.h), so the flag — one per instantiation — needs no lock
template <auto Kern>
hipError_t set_max_dynamic_lds(int bytes) {
  static bool done[64] = {};
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return hipErrorInvalidDevice;
  if (done[dev]) return hipSuccess;
  const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(Kern), hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
  done[dev] = e == hipSuccess;
  return e;
}
// grid of a launch on tiles of BM output channels x BN pixels: blocks of its largest problem (x), K slices of its most split one (z)
struct TileGrid { int maxblocks, zs; };
inline TileGrid tile_grid(const ConvLaunch& L, int BM, int BN) {
  TileGrid g{0, 1};
  for (int i = 0; i < L.nprob; ++i) {
    const ConvProblem& P = L.p[i];
    const int Ptot = P.n_img * P.Hout * P.Wout;
    g.maxblocks = std::max(g.maxblocks, ((Ptot + BN - 1) / BN) * ((P.cout_pad + BM - 1) / BM));
    g.zs = std::max(g.zs, P.nsplit);
  }
  return g;
}
// bf16x3 (opt-in math mode): the launch runs the split-bf16 K loop when every problem of it carries split weights and dispatch.hip
// (select_bf16x3) said so
inline bool launch_runs_bf16x3(const ConvLaunch& L) {
  bool b3 = L.nprob > 0;
  for (int i = 0; i < L.nprob; ++i) b3 = b3 && L.p[i].w3 != nullptr && L.p[i].use_w3;
  return b3;
}

hipError_t set_stamp_buffer_sp(unsigned long long* p);
hipError_t set_stamp_buffer_wino(unsigned long long* p);
hipError_t launch_conv_sp(const ConvLaunch& L, int epi, bool scaled, int bn, hipStream_t stream);
// Winograd kernel (conv_wino.hip).  A workgroup's block: WN_COUT_T output channels x (4 or 2 tile rows) x WN_TW tile columns — 32 or 16
// Winograd tiles.  The form names the run structure of a launch (also the profiler's variant of the kernel key).  dispatch.hip: wino_plan
// decides form, block height, window of tile rows, grid and reciprocals and writes them into the ConvLaunch; the launcher only maps
// (epi, form, block height) to the instantiation (hipErrorInvalidValue where there is none: dilated + blend, sample / LNG on 16-tile
// blocks, SE-scaled concatenated images on 16-tile blocks)
constexpr int WN_COUT_T = 64, WN_TW = 8, WN_TH = 4, WN_TH_SMALL = 2;
enum WinoForm { WINO_PLAIN = 2, WINO_DIL = 3, WINO_CAT = 4 };
// tall: the F(4,3) x F(2,3) arithmetic of the 32-tile plain / concatenated AFFINE and BLEND forms and of the 7x7 LNG tap groups (dispatch.hip: wino_tall decides)
hipError_t launch_conv_wino(const ConvLaunch& L, int epi, WinoForm form, int th, bool tall, hipStream_t stream);
// the packed Winograd weights of a layer: U (16 positions) and behind it U42 (24 positions, the tall form), both [group][cin_pad / 16][position][cout_pad][16];
// floats from sf_conv_w::w_wino to U42, and of both copies together (cout_pad is a multiple of 64: every part stays 256-byte aligned)
__host__ __device__ inline size_t wino_tall_offset(int cout_pad, int cin_pad, int kh) { return (size_t)(kh == 7 ? 9 : 1) * 16 * cout_pad * cin_pad; }
inline size_t wino_pack_floats(int cout_pad, int cin_pad, int kh) { return wino_tall_offset(cout_pad, cin_pad, kh) / 16 * (16 + 24); }
hipError_t launch_wino_weights(const float* w, float* U, int cout_pad, int cin_pad, int ksz, hipStream_t stream);
bool wino_takes_tall(const ConvProblem& q, int epi, WinoForm form, int th);
bool wino_takes(const ConvProblem& q, int epi);
bool wino_same_geometry(const ConvProblem& a, const ConvProblem& b);
void wino_tile_grid(const ConvProblem& q, int& tiles_x, int& tiles_y);
double wino_tiles(const ConvProblem& q);
hipError_t launch_sp_flow(const SpFlow& F, int grid, bool b3, hipStream_t stream);
hipError_t launch_flow_write(const void* host_src, void* dev_dst, size_t bytes, hipStream_t stream);
bool sp_flow_has(int epi, bool scaled, int bn);
int sp_flow_capacity(bool b3);
hipError_t launch_convnext_mlp(const float* t, const float* x, float* out, const float* w1, const float* s1, const float* b1, const float* w2, const float* s2, const float* b2, long P, hipStream_t stream);
hipError_t launch_transpose(const float* in, float* out, int n, int rows, int cols, hipStream_t s);
hipError_t launch_transpose_strided(const float* in, float* out, int n, int rows, int cols, size_t in_stride, size_t out_stride, hipStream_t s);
hipError_t launch_maxpool2(const float* in, float* out, int n, int Hin, int Win, int C, int ceil_pad, hipStream_t s);
hipError_t launch_mean_from_partials(const float* part, float* out, int n, int nslab, int C, int hw, hipStream_t s);
hipError_t launch_logsigmoid(const float* in, float* out, size_t n, hipStream_t s);
hipError_t launch_upsample2(const float* in, float* out, int n, int Hin, int Win, int C, hipStream_t s);
hipError_t launch_broadcast_channels(const float* vec, float* out, int n, int HW, int k, int out_cs, int out_co, hipStream_t s);
hipError_t launch_upsample_bilinear2_add(const float* in, const float* skip, float* out, int n, int Hin, int Win, int C, hipStream_t s);
hipError_t launch_se_fc(const float* chansum, int ntile, int C, int Cr, int hw, const float* fc0, const float* fc2, float* scale, int n_img, hipStream_t s);
hipError_t launch_chan_partial(const float* in, float* part, int n, int HW, int C, int nslab, hipStream_t s);
hipError_t launch_dwconv7_ln(const float* in, float* out, const float* wdw, const float* bdw, const float* lnw, const float* lnb, int n, int H, int W, int C, float eps, hipStream_t s);
hipError_t launch_aspp_pool(const float* in, float* part, float* bias_img, int n, int HW, int C, int hid, const float* w1, const float* s1, const float* b1, const float* wp, const float* ps, const float* pb, int nslab, hipStream_t s);

// ceil(2^32 / d) for the kernels' divisions by multiplication (0 for d <= 1: "divide"); exact while dividend x d < 2^32
inline unsigned magic(long d) { return d <= 1 ? 0u : (unsigned)((0x100000000ull + (unsigned long long)d - 1) / (unsigned long long)d); }
}  // namespace sf
