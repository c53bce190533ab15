// Camera image front end for gfx950 + C ABI (sf_resample_*, sf_image_frontend_*): decoded uint8 frames to the trunk's fp32 input —
// what NuscenesData.get_input_data does between Image.open and the model (streamingflow/datas/NuscenesData.py:251-269):
//   resize   PIL's img.resize(resize_dims, BILINEAR) (streamingflow/utils/geometry.py:9-13).  On a downscale that is an antialiased triangle
//            filter whose support is the scale factor, in 22-bit fixed point, as a horizontal and a vertical pass with a uint8 image between
//            them (Pillow, Resample.c: precompute_coeffs, normalize_coeffs_8bpc, ImagingResampleHorizontal_8bpc / Vertical_8bpc):
//              pass: out = clip8((2^21 + sum_j in[xmin + j] * k[j]) >> 22)
//            The tables are host code below, in double and in Pillow's order of operations: equal, not close.
//   crop     img.crop((l, t, r, b)) in resized coordinates; positions outside the resized image are 0
//   tensor   ToTensor + Normalize: ((float)u / 255 - mean[c]) / std[c], read from a 3 x 256 table the plan holds (computed on the host with
//            IEEE fp32 operations, the values torch computes on the CPU)
// One launch.  A workgroup owns a tile of TH x TW output pixels: it stages the source rows its vertical taps need — the columns its
// horizontal taps need of them, 16 bytes per lane where the rows are 16-byte aligned — into LDS, runs the horizontal pass out of LDS into
// a uint8 LDS image, and the vertical pass out of that.  The intermediate never reaches global memory; source rows the crop drops are
// never read.  At 900x1600 -> 270x480 a tile of 8 rows reads 30 source rows for 26.7 rows' worth of output: 1.13 x vertically, 1.04 x
// horizontally (the L2 serves most of the overlap).  Integer arithmetic throughout, so eager and captured runs are bitwise equal.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>

#include "../../include/sfnative.h"

namespace sf {

constexpr int IF_TW = 64, IF_TH = 8;          // output tile of a workgroup
constexpr int IF_IW = IF_TW * 3;              // bytes of a row of the intermediate
constexpr int IF_THREADS = 256;
constexpr int IF_KREG = 9;                   // taps a lane keeps in registers in the horizontal pass
constexpr int IF_LDS_BUDGET = 40 * 1024;      // raw rows are staged in chunks that keep a workgroup's LDS under this
constexpr int IF_MAGIC = 0x53464946;          // "SFIF"
// plan header, int32 words (the blob is int32 words throughout; the normalise table is fp32 bit patterns)
enum { PH_MAGIC = 0, PH_HS, PH_WS, PH_HR, PH_WR, PH_L, PH_T, PH_W, PH_H, PH_KX, PH_KY, PH_SPAN, PH_RAW_STRIDE, PH_CHUNK, PH_BX, PH_KXT,
       PH_BY, PH_KYT, PH_LUT, PH_WORDS, PH_LDS, PH_VEC, PH_HEADER = 24 };

// The products are byte x coefficient with |coefficient| <= 2^22 (normalised weights in 22-bit fixed point): 24-bit multiplies are exact.
__device__ __forceinline__ int clip8(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

__global__ __launch_bounds__(IF_THREADS) void image_frontend_kernel(const uint8_t* __restrict__ src, const int32_t* __restrict__ plan,
                                                                    float* __restrict__ out, uint8_t* __restrict__ out_u8, int planar,
                                                                    int tiles_x, int tiles_y) {
  extern __shared__ __align__(16) unsigned char lds[];
  const int Hs = plan[PH_HS], Ws = plan[PH_WS], Hr = plan[PH_HR], Wr = plan[PH_WR], l = plan[PH_L], t = plan[PH_T], w = plan[PH_W],
            h = plan[PH_H], kx = plan[PH_KX], ky = plan[PH_KY], span_cap = plan[PH_SPAN], raw_stride = plan[PH_RAW_STRIDE],
            chunk = plan[PH_CHUNK], vec = plan[PH_VEC];
  const int32_t* bx = plan + plan[PH_BX];
  const int32_t* kxt = plan + plan[PH_KXT];
  const int32_t* by = plan + plan[PH_BY];
  const int32_t* kyt = plan + plan[PH_KYT];
  const float* lut_g = reinterpret_cast<const float*>(plan + plan[PH_LUT]);
  // LDS: normalise table [3][256] fp32 | horizontal coefficients [kx][TW] int32 | (xmin, n) of the tile's columns [TW][2] int32 |
  //      vertical coefficients [TH][ky] and (ymin, n) [TH][2] of the tile's rows | intermediate [span_cap][IW] uint8 | raw source rows [chunk][raw_stride] uint8   (every part a multiple of 16 bytes)
  float* lut = reinterpret_cast<float*>(lds);
  int32_t* kxs = reinterpret_cast<int32_t*>(lds + 3072);
  int32_t* bxs = kxs + kx * IF_TW;
  int32_t* kys = bxs + 2 * IF_TW;
  int32_t* bys = kys + IF_TH * ky;
  unsigned char* inter = reinterpret_cast<unsigned char*>(bys + 2 * IF_TH);
  unsigned char* raw = inter + span_cap * IF_IW;

  const int tid = threadIdx.x;
  const int tile = blockIdx.x % (tiles_x * tiles_y), img = blockIdx.x / (tiles_x * tiles_y);
  const int x0 = (tile % tiles_x) * IF_TW, y0 = (tile / tiles_x) * IF_TH;
  const int x1 = min(x0 + IF_TW, w), y1 = min(y0 + IF_TH, h);
  // the part of the tile inside the resized image, in resized coordinates
  const int xa = max(l + x0, 0), xb = min(l + x1, Wr), ya = max(t + y0, 0), yb = min(t + y1, Hr);
  const bool any = xa < xb && ya < yb;

  for (int i = tid; i < 768; i += IF_THREADS) lut[i] = lut_g[i];
  for (int i = tid; i < IF_TH * ky; i += IF_THREADS) {      // rows outside the resized image: zeros, never used
    const int yl = i / ky, ry = t + y0 + yl;
    kys[i] = ry >= 0 && ry < Hr ? kyt[(size_t)ry * ky + (i - yl * ky)] : 0;
  }
  if (tid < 2 * IF_TH) {
    const int ry = t + y0 + (tid >> 1);
    bys[tid] = ry >= 0 && ry < Hr ? by[2 * ry + (tid & 1)] : 0;
  }
  int r0 = 0;
  if (any) {
    const int nxo = xb - xa;                  // columns of the horizontal pass
    const int c0 = bx[2 * xa], c1 = bx[2 * (xb - 1)] + bx[2 * (xb - 1) + 1];      // source columns [c0, c1)
    r0 = by[2 * ya];
    const int r1 = by[2 * (yb - 1)] + by[2 * (yb - 1) + 1];                       // source rows [r0, r1)
    // Up to IF_KREG taps (downscales up to 4 x): a lane keeps one column's coefficients in registers and walks the rows.  More taps: the
    // coefficients of the tile's columns go to LDS and the tap loop runs to each column's own count.
    const bool few = kx <= IF_KREG;
    const int lane_x = tid & (IF_TW - 1), lane_on = few && lane_x < nxo;
    int kreg[IF_KREG], lane_off = 0;
#pragma unroll
    for (int j = 0; j < IF_KREG; ++j) kreg[j] = lane_on && j < kx ? kxt[(size_t)(xa + lane_x) * kx + j] : 0;      // rows are zero past their tap count
    if (!few) {
      for (int i = tid; i < nxo; i += IF_THREADS) {
        bxs[2 * i] = bx[2 * (xa + i)];
        bxs[2 * i + 1] = bx[2 * (xa + i) + 1];
      }
      for (int i = tid; i < kx * nxo; i += IF_THREADS) {
        const int j = i / nxo, xi = i - j * nxo;
        kxs[j * IF_TW + xi] = kxt[(size_t)(xa + xi) * kx + j];
      }
    }
    const size_t row_bytes = (size_t)Ws * 3;
    const uint8_t* simg = src + (size_t)img * Hs * row_bytes;
    const int a0 = vec ? (c0 * 3) & ~15 : c0 * 3;                                  // first staged byte of a source row
    const int nstage = vec ? (c1 * 3 - a0 + 15) >> 4 : (c1 - c0) * 3;             // 16-byte pieces, or bytes, staged per row
    const int col_l = xa - l - x0;            // tile column of the first resized column
    if (lane_on) lane_off = bx[2 * (xa + lane_x)] * 3 - a0;      // the column's first tap in a staged row
    for (int rc = r0; rc < r1; rc += chunk) {
      const int rows = min(chunk, r1 - rc);
      if (vec) {
        for (int i = tid; i < rows * nstage; i += IF_THREADS) {
          const int rr = i / nstage, v = i - rr * nstage;
          const size_t off = (size_t)a0 + 16 * (size_t)v;      // rows are whole 16-byte pieces: a piece that starts inside a row ends inside it
          const uint4 q = *reinterpret_cast<const uint4*>(simg + (size_t)(rc + rr) * row_bytes + off);
          *reinterpret_cast<uint4*>(raw + rr * raw_stride + 16 * v) = q;
        }
      } else {
        for (int i = tid; i < rows * nstage; i += IF_THREADS) {
          const int rr = i / nstage, v = i - rr * nstage;
          raw[rr * raw_stride + v] = simg[(size_t)(rc + rr) * row_bytes + a0 + v];
        }
      }
      __syncthreads();      // raw rows, and before the first chunk the tables, are in LDS
      if (few) {
        // 3 * IF_KREG = 27 bytes from the column's first tap on, read as the 8 aligned words that hold them and shifted into place;
        // taps past the column's count have zero coefficients (what they read is inside the LDS block: 32 spare bytes behind raw)
        if (lane_on) {
          for (int rr = tid >> 6; rr < rows; rr += IF_THREADS / IF_TW) {
            const uint32_t* q = reinterpret_cast<const uint32_t*>(raw + rr * raw_stride + (lane_off & ~3));
            uint32_t wd[8], d[7];
#pragma unroll
            for (int i = 0; i < 8; ++i) wd[i] = q[i];
#pragma unroll
            for (int i = 0; i < 7; ++i) d[i] = __builtin_amdgcn_alignbyte(wd[i + 1], wd[i], lane_off & 3);
            int s[3] = {1 << 21, 1 << 21, 1 << 21};
#pragma unroll
            for (int j = 0; j < IF_KREG; ++j)
#pragma unroll
              for (int c = 0; c < 3; ++c) s[c] += __mul24((int)((d[(3 * j + c) >> 2] >> (8 * ((3 * j + c) & 3))) & 255u), kreg[j]);
            unsigned char* o = inter + (rc - r0 + rr) * IF_IW + (col_l + lane_x) * 3;
            o[0] = (unsigned char)clip8(s[0] >> 22);
            o[1] = (unsigned char)clip8(s[1] >> 22);
            o[2] = (unsigned char)clip8(s[2] >> 22);
          }
        }
      } else {
        for (int i = tid; i < rows * nxo; i += IF_THREADS) {
        const int rr = i / nxo, xi = i - rr * nxo;
        const unsigned char* p = raw + rr * raw_stride + (bxs[2 * xi] * 3 - a0);
        const int nt = bxs[2 * xi + 1];
        int s0 = 1 << 21, s1 = 1 << 21, s2 = 1 << 21;
        for (int j = 0; j < nt; ++j) {
          const int k = kxs[j * IF_TW + xi];
          s0 += __mul24((int)p[3 * j], k);
          s1 += __mul24((int)p[3 * j + 1], k);
          s2 += __mul24((int)p[3 * j + 2], k);
        }
        unsigned char* q = inter + (rc - r0 + rr) * IF_IW + (col_l + xi) * 3;
        q[0] = (unsigned char)clip8(s0 >> 22);
        q[1] = (unsigned char)clip8(s1 >> 22);
        q[2] = (unsigned char)clip8(s2 >> 22);
        }
      }
      __syncthreads();      // the intermediate rows of this chunk are written; raw may be overwritten
    }
  } else {
    __syncthreads();        // the normalise table and the rows' coefficients
  }

  // vertical pass, crop padding, normalise.  Lanes run along what is contiguous in `out`: x (planar) or (x, c)
  for (int e = tid; e < IF_TH * IF_IW; e += IF_THREADS) {
    int yl, xl, c;
    if (planar) {
      xl = e % IF_TW;
      c = (e / IF_TW) % 3;
      yl = e / IF_IW;
    } else {
      c = e % 3;
      xl = (e / 3) % IF_TW;
      yl = e / IF_IW;
    }
    const int oy = y0 + yl, ox = x0 + xl;
    if (oy >= h || ox >= w) continue;
    const int ry = t + oy, rx = l + ox;
    int u = 0;
    if (ry >= 0 && ry < Hr && rx >= 0 && rx < Wr) {
      const int base = bys[2 * yl] - r0, nt = bys[2 * yl + 1];      // first intermediate row of this output row's taps
      const int32_t* k = kys + yl * ky;
      const unsigned char* p = inter + xl * 3 + c;
      int s = 1 << 21;
      if (ky <= IF_KREG) {      // all nine taps at once: coefficients past the row's count are zero, their rows clamped into the image
#pragma unroll
        for (int j = 0; j < IF_KREG; ++j) s += __mul24((int)p[min(base + j, span_cap - 1) * IF_IW], j < ky ? k[j] : 0);
      } else {
        for (int j = 0; j < nt; ++j) s += __mul24((int)p[(base + j) * IF_IW], k[j]);
      }
      u = clip8(s >> 22);
    }
    const float v = lut[c * 256 + u];
    const size_t pix = (size_t)oy * w + ox;
    if (planar) out[((size_t)img * 3 + c) * h * w + pix] = v;
    else out[((size_t)img * h * w + pix) * 3 + c] = v;
    if (out_u8) out_u8[((size_t)img * h * w + pix) * 3 + c] = (uint8_t)u;
  }
}

// ---- host: the tables ------------------------------------------------------------------------------------------------------------------
// Pillow computes these in double and without fused multiply-adds; a contraction would change a weight's last bit now and then.
#pragma clang fp contract(off)

static int resample_ksize(int in_size, int out_size) {
  const double scale = (double)in_size / out_size;
  const double filterscale = scale < 1.0 ? 1.0 : scale;
  const double support = 1.0 * filterscale;
  const double taps = std::ceil(support) * 2 + 1;
  return taps > 1e6 ? 1000000 : (int)taps;
}

// bounds [out_size][2], k [out_size][ksize] (rows zero-filled past n): precompute_coeffs + normalize_coeffs_8bpc for the BILINEAR filter
static void resample_table(int in_size, int out_size, int ksize, int32_t* bounds, int32_t* k) {
  const double scale = (double)in_size / out_size;
  const double filterscale = scale < 1.0 ? 1.0 : scale;
  const double support = 1.0 * filterscale;
  const double ss = 1.0 / filterscale;
  for (int xx = 0; xx < out_size; ++xx) {
    const double center = (xx + 0.5) * scale;
    int xmin = (int)(center - support + 0.5);
    if (xmin < 0) xmin = 0;
    int xmax = (int)(center + support + 0.5);
    if (xmax > in_size) xmax = in_size;
    const int n = xmax - xmin;
    int32_t* row = k + (size_t)xx * ksize;
    double ww = 0.0;
    for (int x = 0; x < n; ++x) {
      double a = (x + xmin - center + 0.5) * ss;
      if (a < 0.0) a = -a;
      ww += a < 1.0 ? 1.0 - a : 0.0;
    }
    for (int x = 0; x < ksize; ++x) {
      if (x >= n) {
        row[x] = 0;
        continue;
      }
      double a = (x + xmin - center + 0.5) * ss;
      if (a < 0.0) a = -a;
      double wgt = a < 1.0 ? 1.0 - a : 0.0;
      if (ww != 0.0) wgt /= ww;
      row[x] = wgt < 0 ? (int)(-0.5 + wgt * (1 << 22)) : (int)(0.5 + wgt * (1 << 22));
    }
    bounds[2 * xx] = xmin;
    bounds[2 * xx + 1] = n;
  }
}

static int align16(long v) { return (int)((v + 15) & ~15L); }

struct FrontendLayout {
  int kx, ky, words, bx, kxt, by, kyt, lut;
};

// SF_OK and the layout, or the status the plan calls report
static int frontend_layout(int Hs, int Ws, int Hr, int Wr, int l, int t, int r, int b, FrontendLayout* L) {
  if (Hs < 1 || Ws < 1 || Hr < 1 || Wr < 1 || r <= l || b <= t) return SF_ERR_INVALID;
  const long lim = 1L << 15;      // every size and crop coordinate stays far inside int arithmetic
  if (Hs > lim || Ws > lim || Hr > lim || Wr > lim || l < -lim || t < -lim || r > 2 * lim || b > 2 * lim) return SF_ERR_INVALID;
  L->kx = resample_ksize(Ws, Wr);
  L->ky = resample_ksize(Hs, Hr);
  if (L->kx > SF_IMAGE_FRONTEND_MAX_TAPS || L->ky > SF_IMAGE_FRONTEND_MAX_TAPS) return SF_ERR_UNSUPPORTED;
  int o = PH_HEADER;
  L->bx = o, o += 2 * Wr;
  L->kxt = o, o += Wr * L->kx;
  L->by = o, o += 2 * Hr;
  L->kyt = o, o += Hr * L->ky;
  o = (o + 3) & ~3;
  L->lut = o, o += 768;
  L->words = o;
  return SF_OK;
}

}  // namespace sf

extern "C" {

int sf_resample_ksize(int in_size, int out_size) {
  if (in_size < 1 || out_size < 1) return 0;
  return sf::resample_ksize(in_size, out_size);
}

int sf_resample_table(int in_size, int out_size, int32_t* bounds, int32_t* k) {
  if (in_size < 1 || out_size < 1 || !bounds || !k) return SF_ERR_INVALID;
  const int ksize = sf::resample_ksize(in_size, out_size);
  if (ksize > SF_IMAGE_FRONTEND_MAX_TAPS) return SF_ERR_UNSUPPORTED;
  sf::resample_table(in_size, out_size, ksize, bounds, k);
  return SF_OK;
}

size_t sf_image_frontend_plan_bytes(int Hs, int Ws, int Hr, int Wr, int l, int t, int r, int b) {
  sf::FrontendLayout L;
  return sf::frontend_layout(Hs, Ws, Hr, Wr, l, t, r, b, &L) == SF_OK ? (size_t)L.words * 4 : 0;
}

int sf_image_frontend_plan(int Hs, int Ws, int Hr, int Wr, int l, int t, int r, int b, const float* mean, const float* std, void* host_blob,
                           size_t blob_bytes) {
  using namespace sf;
  FrontendLayout L;
  const int st = frontend_layout(Hs, Ws, Hr, Wr, l, t, r, b, &L);
  if (st != SF_OK) return st;
  if (!mean || !std || !host_blob || blob_bytes < (size_t)L.words * 4) return SF_ERR_INVALID;
  int32_t* p = static_cast<int32_t*>(host_blob);
  std::memset(p, 0, (size_t)L.words * 4);
  resample_table(Ws, Wr, L.kx, p + L.bx, p + L.kxt);
  resample_table(Hs, Hr, L.ky, p + L.by, p + L.kyt);
  // ToTensor + Normalize of every byte value: two IEEE fp32 divisions and a subtraction, each rounded (volatile: no folding into one)
  float* lut = reinterpret_cast<float*>(p + L.lut);
  for (int c = 0; c < 3; ++c)
    for (int u = 0; u < 256; ++u) {
      volatile float v = (float)u / 255.0f;
      v = v - mean[c];
      v = v / std[c];
      lut[c * 256 + u] = v;
    }
  // the largest block of source rows and columns any tile stages
  const int w = r - l, h = b - t;
  const int32_t* bx = p + L.bx;
  const int32_t* by = p + L.by;
  int span = 1, cols = 1;
  for (int y0 = 0; y0 < h; y0 += IF_TH) {
    const int ya = t + y0 > 0 ? t + y0 : 0, y1 = y0 + IF_TH < h ? y0 + IF_TH : h, yb = t + y1 < Hr ? t + y1 : Hr;
    if (ya < yb) {
      const int s = by[2 * (yb - 1)] + by[2 * (yb - 1) + 1] - by[2 * ya];
      span = s > span ? s : span;
    }
  }
  for (int x0 = 0; x0 < w; x0 += IF_TW) {
    const int xa = l + x0 > 0 ? l + x0 : 0, x1 = x0 + IF_TW < w ? x0 + IF_TW : w, xb = l + x1 < Wr ? l + x1 : Wr;
    if (xa < xb) {
      const int s = bx[2 * (xb - 1)] + bx[2 * (xb - 1) + 1] - bx[2 * xa];
      cols = s > cols ? s : cols;
    }
  }
  const int raw_stride = align16((long)cols * 3 + 30);      // up to 15 bytes in front (alignment of the first piece) and 15 behind
  const int fixed = 3072 + L.kx * IF_TW * 4 + 2 * IF_TW * 4 + IF_TH * (L.ky + 2) * 4 + span * IF_IW;
  int chunk = (IF_LDS_BUDGET - fixed) / raw_stride;
  chunk = chunk < 1 ? 1 : (chunk > span ? span : chunk);
  const long lds = (long)fixed + (long)chunk * raw_stride + 32;      // + what the register form of the horizontal pass may read past a row
  if (lds > 64 * 1024) return SF_ERR_UNSUPPORTED;
  p[PH_MAGIC] = IF_MAGIC, p[PH_HS] = Hs, p[PH_WS] = Ws, p[PH_HR] = Hr, p[PH_WR] = Wr, p[PH_L] = l, p[PH_T] = t, p[PH_W] = w, p[PH_H] = h;
  p[PH_KX] = L.kx, p[PH_KY] = L.ky, p[PH_SPAN] = span, p[PH_RAW_STRIDE] = raw_stride, p[PH_CHUNK] = chunk;
  p[PH_BX] = L.bx, p[PH_KXT] = L.kxt, p[PH_BY] = L.by, p[PH_KYT] = L.kyt, p[PH_LUT] = L.lut, p[PH_WORDS] = L.words, p[PH_LDS] = (int)lds;
  p[PH_VEC] = ((long)Ws * 3) % 16 == 0;      // rows of whole 16-byte pieces: staged 16 bytes per lane (the forward call checks src's alignment)
  return SF_OK;
}

int sf_image_frontend_fwd(const uint8_t* src, const void* plan_host, const void* plan_dev, float* out, int planar, uint8_t* out_u8, int n,
                          int Hs, int Ws, int h, int w, void* stream) {
  using namespace sf;
  if (!src || !plan_host || !plan_dev || !out || n < 1 || Hs < 1 || Ws < 1 || h < 1 || w < 1) return SF_ERR_INVALID;
  const int32_t* p = static_cast<const int32_t*>(plan_host);
  if (p[PH_MAGIC] != IF_MAGIC || p[PH_HS] != Hs || p[PH_WS] != Ws || p[PH_H] != h || p[PH_W] != w) return SF_ERR_INVALID;
  // the 16-byte form reads whole pieces of a row: the rows are 16-byte multiples (the plan's flag) and src must be aligned too
  if (p[PH_VEC] && (reinterpret_cast<uintptr_t>(src) & 15)) return SF_ERR_INVALID;
  if ((reinterpret_cast<uintptr_t>(plan_dev) & 15) || (reinterpret_cast<uintptr_t>(out) & 3)) return SF_ERR_INVALID;
  const int tiles_x = (w + IF_TW - 1) / IF_TW, tiles_y = (h + IF_TH - 1) / IF_TH;
  const long blocks = (long)tiles_x * tiles_y * n;
  if (blocks >= (1L << 31)) return SF_ERR_INVALID;
  hipLaunchKernelGGL(image_frontend_kernel, dim3((unsigned)blocks), dim3(IF_THREADS), (size_t)p[PH_LDS], static_cast<hipStream_t>(stream), src,
                     static_cast<const int32_t*>(plan_dev), out, out_u8, planar, tiles_x, tiles_y);
  return hipGetLastError() == hipSuccess ? SF_OK : SF_ERR_LAUNCH;
}

}  // extern "C"
