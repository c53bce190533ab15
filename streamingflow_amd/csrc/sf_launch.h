// Host launchers of the kernel files, declared once: every .hip file that defines one and every caller includes this header, so a changed
// signature fails to compile instead of failing to link.
#pragma once
#include "sf_device.h"

namespace sf {
hipError_t launch_conv(const ConvLaunch& L, int epi, int cfg, hipStream_t stream);
hipError_t launch_conv_direct(const ConvLaunch& L, int epi, int mt, int ks, hipStream_t stream);
hipError_t launch_conv_glds(const ConvLaunch& L, int epi, int tile, int variant, hipStream_t stream);
hipError_t set_stamp_buffer(unsigned long long* p);
int glds_occupancy(int which);
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
// tall: the F(4,3) x F(2,3) arithmetic of the 32-tile plain / concatenated AFFINE and BLEND forms (dispatch.hip: wino_tall decides)
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
