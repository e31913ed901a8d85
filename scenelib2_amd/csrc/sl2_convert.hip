// Raw camera frames of a whole batch -> the engine's grey images, in one launch (the arithmetic:
// sl2_convert_dev.hpp).  In front of the step, like the reference's UsbCamGrabber in front of GoOneStep - not part of it.
//
// k_convert_frames: a workgroup of 256 threads owns one sequence and a band of kConvBandRows output rows.  It lists the source
// rows the band's row taps name (each once; rows no tap names are never read), streams them in with 16-byte loads - a scalar
// head and tail where the row's address or length breaks the alignment -, reduces them to grey in LDS, forms the outputs from
// LDS and stores four output bytes per lane.  Sequences of any source size and format share the launch: the grid is sized by
// the OUTPUT rows, which are the same for all of them.
// k_convert_area, k_raw_linear, k_raw_area: the SL2_RESIZE_AREA sequences and those of a deep grey or Bayer format, listed on the
// device, a launch each where there are any.
// k_convert_remap (sl2_convert_remap.hip, a unit of its own so that this unit's device code is the same with and without it): the
// sequences that follow a per-pixel map (the lens remap), listed likewise; a gather, nothing staged.
// Which of the five owns a sequence, the lists and every launch's size: sl2_convert_plan.hpp (convert_route, convert_plan).
#include "sl2_common.hpp"
#include "sl2_convert_dev.hpp"
#include "sl2_convert_plan.hpp"
#include "sl2_convert_remap.hpp"

namespace sl2 {

// (kConvThreads, kConvBandRows, the LDS sizes and the route bits of the device records: sl2_convert_plan.hpp)

struct ConvArgs {
  const sl2_frame_source* src;   // [nseq]
  const uint32_t* taps;          // [nseq][tap_stride]: col_taps column taps (out_w rounded up to 4, the rest 0), then out_h row taps
  const uint8_t* raw;
  uint8_t* out;
  unsigned long long seq_stride;
  int out_w, out_h, col_taps, tap_stride, bands;
};

template <int FMT> struct ConvFmt;
template <> struct ConvFmt<SL2_PIX_GRAY8> { static constexpr int kGroup = 16, kBytes = 16; };
template <> struct ConvFmt<SL2_PIX_RGB24> { static constexpr int kGroup = 16, kBytes = 48; };
template <> struct ConvFmt<SL2_PIX_BGR24> { static constexpr int kGroup = 16, kBytes = 48; };
template <> struct ConvFmt<SL2_PIX_UYVY> { static constexpr int kGroup = 8, kBytes = 16; };
template <> struct ConvFmt<SL2_PIX_YUYV> { static constexpr int kGroup = 8, kBytes = 16; };
template <> struct ConvFmt<SL2_PIX_GRAY10> { static constexpr int kGroup = 8, kBytes = 16; };      // a 16-byte load is 8 pixels
template <> struct ConvFmt<SL2_PIX_GRAY12> { static constexpr int kGroup = 8, kBytes = 16; };
template <> struct ConvFmt<SL2_PIX_GRAY16> { static constexpr int kGroup = 8, kBytes = 16; };

struct ConvShared {
  alignas(16) uint8_t grey[kConvLdsBytes];
  int row[kConvSlots];      // the source row a slot holds
  int head[kConvSlots];     // pixels before the first aligned group (scalar)
  int first[kConvSlots];    // byte offset of the first aligned group in the row
  int groups[kConvSlots];   // aligned groups (one lane each)
  int shift[kConvSlots];    // where the row's pixel 0 sits in its slot: head + shift is a multiple of the group
  int slot0[kConvBandRows], slot1[kConvBandRows];
  uint32_t rtap[kConvBandRows];   // the band's row taps
  int nslots;
};

__device__ __forceinline__ uint32_t conv_byte(const uint32_t* w, int k) { return (w[k >> 2] >> (8 * (k & 3))) & 255u; }

// Stage the listed source rows as grey bytes: slot k of grey holds row sh.row[k] from byte sh.shift[k] on.  (ROWS: ConvShared
// with its own grey, or the RawRows of a Bayer sub-pass with the raw stage.)
template <int FMT, typename ROWS>
__device__ __forceinline__ void conv_stage(ROWS& sh, uint8_t* grey, const uint8_t* __restrict__ base, int pitch, int W, int wpad) {
  constexpr int G = ConvFmt<FMT>::kGroup, VB = ConvFmt<FMT>::kBytes;
  const int tid = threadIdx.x;
  const int nslots = sh.nslots;
  const int row_bytes = W * convert_bpp(FMT);
  if (tid < nslots) {
    const unsigned a = (unsigned)(uintptr_t)(base + (size_t)sh.row[tid] * (size_t)pitch);
    int head, first, groups;
    if (FMT == SL2_PIX_GRAY8) {
      head = (int)((0u - a) & 15u); first = head;
    } else if (FMT == SL2_PIX_RGB24 || FMT == SL2_PIX_BGR24) {
      head = (int)(((0u - a) * 11u) & 15u); first = 3 * head;      // a + 3 head = 0 mod 16 (3 * 11 = 1 mod 16)
    } else {
      first = (int)((0u - a) & 15u);
      head = (first - (FMT == SL2_PIX_UYVY ? 1 : 0) + 1) >> 1;     // pixels whose Y byte lies before `first` (deep grey: `first` is even)
    }
    if (head >= W) { head = W; groups = 0; }
    else if (convert_is_422(FMT) || convert_is_deep(FMT)) groups = row_bytes > first ? (row_bytes - first) / 16 : 0;
    else groups = (W - head) / G;
    sh.head[tid] = head; sh.first[tid] = first; sh.groups[tid] = groups; sh.shift[tid] = (G - head % G) % G;
  }
  __syncthreads();
  // the aligned middle: one group per lane
  const int gmax = row_bytes / VB + 1;      // groups of a row, at most
  for (int idx = tid; idx < nslots * gmax; idx += kConvThreads) {
    const int k = idx / gmax, c = idx - k * gmax;
    if (c >= sh.groups[k]) continue;
    const uint8_t* rp = base + (size_t)sh.row[k] * (size_t)pitch + sh.first[k] + c * VB;
    uint8_t* dst = grey + k * wpad + sh.shift[k] + sh.head[k] + c * G;
    if (FMT == SL2_PIX_GRAY8) {
      *reinterpret_cast<uint4*>(dst) = *reinterpret_cast<const uint4*>(rp);
    } else if (FMT == SL2_PIX_UYVY || FMT == SL2_PIX_YUYV) {
      const uint4 v = *reinterpret_cast<const uint4*>(rp);
      // Y sits at the odd bytes of the ROW for UYVY, at the even ones for YUYV: in the chunk, at byte (ypos ^ first) & 1 of every pair
      const int s8 = 8 * (((FMT == SL2_PIX_UYVY ? 1 : 0) ^ sh.first[k]) & 1);
      const uint32_t t0 = v.x >> s8, t1 = v.y >> s8, t2 = v.z >> s8, t3 = v.w >> s8;
      uint2 o;
      o.x = (t0 & 255u) | ((t0 >> 8) & 0xff00u) | ((t1 & 255u) << 16) | ((t1 << 8) & 0xff000000u);
      o.y = (t2 & 255u) | ((t2 >> 8) & 0xff00u) | ((t3 & 255u) << 16) | ((t3 << 8) & 0xff000000u);
      *reinterpret_cast<uint2*>(dst) = o;
    } else if (convert_is_deep(FMT)) {
      const uint4 v = *reinterpret_cast<const uint4*>(rp);      // eight words of 16 bits
      constexpr int N = FMT == SL2_PIX_GRAY10 ? 10 : FMT == SL2_PIX_GRAY12 ? 12 : 16;
      uint2 o;
      o.x = (uint32_t)convert_deep_grey(N, v.x) | ((uint32_t)convert_deep_grey(N, v.x >> 16) << 8) |
            ((uint32_t)convert_deep_grey(N, v.y) << 16) | ((uint32_t)convert_deep_grey(N, v.y >> 16) << 24);
      o.y = (uint32_t)convert_deep_grey(N, v.z) | ((uint32_t)convert_deep_grey(N, v.z >> 16) << 8) |
            ((uint32_t)convert_deep_grey(N, v.w) << 16) | ((uint32_t)convert_deep_grey(N, v.w >> 16) << 24);
      *reinterpret_cast<uint2*>(dst) = o;
    } else {
      uint32_t w[12];
      const uint4 v0 = reinterpret_cast<const uint4*>(rp)[0], v1 = reinterpret_cast<const uint4*>(rp)[1], v2 = reinterpret_cast<const uint4*>(rp)[2];
      w[0] = v0.x; w[1] = v0.y; w[2] = v0.z; w[3] = v0.w; w[4] = v1.x; w[5] = v1.y; w[6] = v1.z; w[7] = v1.w;
      w[8] = v2.x; w[9] = v2.y; w[10] = v2.z; w[11] = v2.w;
      uint32_t o[4] = {0, 0, 0, 0};
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int c0 = (int)conv_byte(w, 3 * i), c1 = (int)conv_byte(w, 3 * i + 1), c2 = (int)conv_byte(w, 3 * i + 2);
        const int g = FMT == SL2_PIX_RGB24 ? convert_rgb_grey(c0, c1, c2) : convert_rgb_grey(c2, c1, c0);
        o[i >> 2] |= (uint32_t)g << (8 * (i & 3));
      }
      *reinterpret_cast<uint4*>(dst) = make_uint4(o[0], o[1], o[2], o[3]);
    }
  }
  // head and tail, a pixel per lane: at most 15 pixels each
  for (int idx = tid; idx < nslots * 32; idx += kConvThreads) {
    const int k = idx >> 5, j = idx & 31;
    const int p = j < 16 ? j : sh.head[k] + sh.groups[k] * G + (j - 16);
    if (j < 16 ? p >= sh.head[k] : p >= W) continue;
    const uint8_t* rp = base + (size_t)sh.row[k] * (size_t)pitch;
    grey[k * wpad + sh.shift[k] + p] = (uint8_t)convert_grey(FMT, rp, p);
  }
}

// The raw rows of a Bayer sub-pass, under the names conv_stage reads, and where each grey slot finds its three
struct RawRows {
  int row[kRawSlots], head[kRawSlots], first[kRawSlots], groups[kRawSlots], shift[kRawSlots];
  int nb[kConvSlots][3];      // the raw slots of rows y - 1, y, y + 1 (reflected) of a grey slot
  int nslots, k1;             // raw rows listed; the first grey slot this sub-pass does not form
};

// What the two raw kernels add to a workgroup's LDS: the dynamic part holds the raw stage (raw_lds bytes: 0 with no Bayer source)
struct RawStage {
  RawRows* rows;
  uint8_t* bytes;
  int raw_lds;
};

// Bayer: grey rows sh.row[0 .. nslots) of source columns xs .. xs + Wp - 1 into the slots of sh.grey, pixel xs at byte 0 of its
// slot.  src0: the source's pixel (0,0).  In sub-passes of as many grey slots as their raw rows fit the raw stage (each raw row
// once per sub-pass: a row two sub-passes share is read again, from L2): thread 0 lists the raw rows, conv_stage brings them in as
// GRAY8 rows - columns xs - 1 .. xs + Wp where the image has them, every load inside the row -, and a lane forms four grey pixels
// from the 3 x 6 raw bytes around them.  Reflection is in the indices: nothing outside the image is ever addressed.
__device__ __forceinline__ void raw_stage_bayer(ConvShared& sh, const RawStage& rs, const uint8_t* __restrict__ src0, int pitch, int W, int H,
                                                int xs, int Wp, int wpad, int fmt) {
  const int tid = threadIdx.x;
  RawRows& rr = *rs.rows;
  const int rx0 = xs > 0 ? xs - 1 : 0, rx1 = xs + Wp < W ? xs + Wp : W - 1;      // the raw columns staged
  const int Wr = rx1 - rx0 + 1, rpad = conv_row_pad(Wr);
  const int fit = rs.raw_lds / rpad;                                             // raw rows the stage holds: at least 4
  const int rcap = fit < kRawSlots ? fit : kRawSlots;
  const int nslots = sh.nslots;
  const int nq = (Wp + 3) >> 2;
  if (tid < nslots) sh.shift[tid] = 0;
  for (int k0 = 0; k0 < nslots;) {
    if (tid == 0) {
      int n = 0, k = k0;
      for (; k < nslots; ++k) {
        const int y = sh.row[k];
        const int ys[3] = {convert_reflect(y - 1, H), y, convert_reflect(y + 1, H)};
        int m = n, at[3];
        bool fits = true;
        for (int j = 0; j < 3 && fits; ++j) {
          int f = -1;
          for (int i = m - 1; i >= 0 && i >= m - 4; --i) if (rr.row[i] == ys[j]) f = i;      // the listed rows only move forward
          if (f < 0) { if (m == rcap) { fits = false; break; } rr.row[m] = ys[j]; f = m++; }
          at[j] = f;
        }
        if (!fits) break;      // (never the sub-pass's first slot: three rows fit an empty stage)
        n = m;
        rr.nb[k][0] = at[0]; rr.nb[k][1] = at[1]; rr.nb[k][2] = at[2];
      }
      rr.nslots = n; rr.k1 = k;
    }
    __syncthreads();
    const int k1 = rr.k1;
    conv_stage<SL2_PIX_GRAY8>(rr, rs.bytes, src0 + rx0, pitch, Wr, rpad);
    __syncthreads();
    for (int idx = tid; idx < (k1 - k0) * nq; idx += kConvThreads) {
      const int k = k0 + idx / nq, q = idx - (k - k0) * nq;
      const int y = sh.row[k], x4 = xs + 4 * q;
      int col[6];      // where raw columns x4 - 1 .. x4 + 4 sit in a staged row (the padding past the row's end: any staged column)
#pragma unroll
      for (int j = 0; j < 6; ++j) {
        int x = x4 - 1 + j;
        x = x < xs + Wp ? convert_reflect(x, W) : convert_reflect(xs + Wp, W);
        col[j] = x - rx0;
      }
      int p[3][6];
#pragma unroll
      for (int r = 0; r < 3; ++r) {
        const int a = rr.nb[k][r];
        const uint8_t* row = rs.bytes + a * rpad + rr.shift[a];
#pragma unroll
        for (int j = 0; j < 6; ++j) p[r][j] = row[col[j]];
      }
      uint32_t packed = 0;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int g = convert_bayer_grey(fmt, p[1][i + 1], p[1][i] + p[1][i + 2], p[0][i + 1] + p[2][i + 1],
                                         p[0][i] + p[0][i + 2] + p[2][i] + p[2][i + 2], x4 + i, y);
        packed |= (uint32_t)g << (8 * i);
      }
      *reinterpret_cast<uint32_t*>(sh.grey + k * wpad + 4 * q) = packed;      // wpad >= Wp + 15: the word stays in its slot
    }
    __syncthreads();      // the next sub-pass overwrites the raw stage
    k0 = k1;
  }
}

// The listed grey rows of a deep grey or Bayer source: what conv_stage is to the other formats
__device__ __forceinline__ void raw_stage(ConvShared& sh, const RawStage& rs, const uint8_t* __restrict__ src0, int pitch, int W, int H, int xs,
                                          int Wp, int wpad, int fmt) {
  switch (fmt) {
    case SL2_PIX_GRAY10: conv_stage<SL2_PIX_GRAY10>(sh, sh.grey, src0 + 2 * (size_t)xs, pitch, Wp, wpad); break;
    case SL2_PIX_GRAY12: conv_stage<SL2_PIX_GRAY12>(sh, sh.grey, src0 + 2 * (size_t)xs, pitch, Wp, wpad); break;
    case SL2_PIX_GRAY16: conv_stage<SL2_PIX_GRAY16>(sh, sh.grey, src0 + 2 * (size_t)xs, pitch, Wp, wpad); break;
    default: raw_stage_bayer(sh, rs, src0, pitch, W, H, xs, Wp, wpad, fmt); break;
  }
}

// The linear kernels' body.  RAW: k_raw_linear's (deep grey and Bayer sequences), else k_convert_frames' (the five 8-bit formats);
// each leaves the other's sequences, and the area kernels', on the scalar branch after its record load.  (A and rs by value: by
// reference k_convert_frames came out with two more scalars parked in vector lanes than it had as a kernel of its own.)
template <bool RAW>
__device__ __forceinline__ void conv_linear(ConvShared& sh, const ConvArgs A, int s, int band, const RawStage rs) {
  const int tid = threadIdx.x;
  const uint32_t* __restrict__ ctab = A.taps + (size_t)s * A.tap_stride;
  const uint32_t* __restrict__ rtab = ctab + A.col_taps;
  const int band0 = band * kConvBandRows;
  const int band_end = band0 + kConvBandRows < A.out_h ? band0 + kConvBandRows : A.out_h;
  const int nq = (A.out_w + 3) >> 2;                                           // four output pixels per lane
  const int qs = nq < kConvThreads ? nq : kConvThreads;
  const int rl = kConvThreads / qs;                                            // output rows formed side by side
  const int tq = tid % qs, tr = tid / qs;
  // everything that does not depend on the source goes out in ONE round trip to memory, beside the source's record: the band's
  // row taps (to LDS) and this lane's first column taps
  if (tid < band_end - band0) sh.rtap[tid] = rtab[band0 + tid];
  uint4 ct_first = make_uint4(0, 0, 0, 0);
  if (tr < rl) ct_first = *reinterpret_cast<const uint4*>(ctab + 4 * tq);
  const sl2_frame_source src = A.src[s];
  const int W = src.width, H = src.height, pitch = src.pitch, fmt = RAW ? src.format & kConvFormatMask : src.format;
  // another kernel's sequence (uniform: a scalar branch): k_convert_area's, or one whose format is the other linear kernel's
  if ((src.format & (kConvAreaBit | kConvRawBit)) != (RAW ? kConvRawBit : 0)) return;
  const uint8_t* __restrict__ base = A.raw + src.offset;
  uint8_t* __restrict__ out = A.out + (size_t)s * A.seq_stride;
  const int wpad = conv_row_pad(W);
  const int cap = kConvLdsBytes / wpad;                                        // rows the LDS holds: at least 4
  const int rmax = cap / 2 < kConvBandRows ? cap / 2 : kConvBandRows;          // output rows per pass: at least 2
  __syncthreads();

  for (int d0 = band0; d0 < band_end; d0 += rmax) {
    const int rr = band_end - d0 < rmax ? band_end - d0 : rmax;
    // the source rows this pass needs, each once.  The rows the taps name only ever move forward by whole rows, so a row is
    // either one of the two listed last or a new one.
    if (tid == 0) {
      int n = 0, ra = -1, rb = -1, sa = 0, sb = 0;
      for (int dl = 0; dl < rr; ++dl) {
        int y0, b0, b1;
        convert_unpack_tap(sh.rtap[d0 - band0 + dl], &y0, &b0, &b1);
        const int y1 = y0 + 1 < H ? y0 + 1 : H - 1;
        int s0, s1;
        if (y0 == ra) s0 = sa; else if (y0 == rb) s0 = sb; else { s0 = n; sh.row[n++] = y0; ra = rb; sa = sb; rb = y0; sb = s0; }
        if (y1 == ra) s1 = sa; else if (y1 == rb) s1 = sb; else { s1 = n; sh.row[n++] = y1; ra = rb; sa = sb; rb = y1; sb = s1; }
        sh.slot0[dl] = s0; sh.slot1[dl] = s1;
      }
      sh.nslots = n;
    }
    __syncthreads();
    if (RAW) raw_stage(sh, rs, base, pitch, W, H, 0, W, wpad, fmt);
    else switch (fmt) {
      case SL2_PIX_GRAY8: conv_stage<SL2_PIX_GRAY8>(sh, sh.grey, base, pitch, W, wpad); break;
      case SL2_PIX_RGB24: conv_stage<SL2_PIX_RGB24>(sh, sh.grey, base, pitch, W, wpad); break;
      case SL2_PIX_BGR24: conv_stage<SL2_PIX_BGR24>(sh, sh.grey, base, pitch, W, wpad); break;
      case SL2_PIX_UYVY: conv_stage<SL2_PIX_UYVY>(sh, sh.grey, base, pitch, W, wpad); break;
      default: conv_stage<SL2_PIX_YUYV>(sh, sh.grey, base, pitch, W, wpad); break;
    }
    __syncthreads();
    if (tr < rl) {
      for (int q = tq; q < nq; q += qs) {
        const uint4 ct = q == tq ? ct_first : *reinterpret_cast<const uint4*>(ctab + 4 * q);
        const uint32_t cw[4] = {ct.x, ct.y, ct.z, ct.w};
        int x0[4], x1[4], a0[4], a1[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          convert_unpack_tap(cw[i], &x0[i], &a0[i], &a1[i]);
          x1[i] = x0[i] + 1 < W ? x0[i] + 1 : W - 1;
        }
        for (int dl = tr; dl < rr; dl += rl) {
          int y0, b0, b1;
          convert_unpack_tap(sh.rtap[d0 - band0 + dl], &y0, &b0, &b1);
          const int k0 = sh.slot0[dl], k1 = sh.slot1[dl];
          const uint8_t* g0 = sh.grey + k0 * wpad + sh.shift[k0];
          const uint8_t* g1 = sh.grey + k1 * wpad + sh.shift[k1];
          uint32_t packed = 0;
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const int h0 = convert_hpass(g0[x0[i]], g0[x1[i]], a0[i], a1[i]);
            const int h1 = convert_hpass(g1[x0[i]], g1[x1[i]], a0[i], a1[i]);
            packed |= (uint32_t)convert_vpass(h0, h1, b0, b1) << (8 * i);
          }
          uint8_t* op = out + (size_t)(d0 + dl) * A.out_w + 4 * q;
          const int left = A.out_w - 4 * q;
          if (left >= 4 && ((uintptr_t)op & 3) == 0) {
            *reinterpret_cast<uint32_t*>(op) = packed;
          } else {
            for (int i = 0; i < 4 && i < left; ++i) op[i] = (uint8_t)(packed >> (8 * i));
          }
        }
      }
    }
    __syncthreads();      // the next pass overwrites the slots
  }
}

__global__ void __launch_bounds__(kConvThreads, 8) k_convert_frames(const ConvArgs A) {
  __shared__ ConvShared sh;
  const int s = blockIdx.x / A.bands;
  conv_linear<false>(sh, A, s, blockIdx.x - s * A.bands, RawStage{nullptr, nullptr, 0});
}

// k_raw_linear: the same for the listed sequences, those of a deep grey or Bayer format under SL2_RESIZE_LINEAR.  Only the staging
// differs (conv_stage's deep grey forms: a 16-byte load is 8 pixels; raw_stage_bayer).  Budget: ConvShared and RawRows, 17 KB of
// static LDS, plus the raw stage (dynamic: eighteen raw rows of the widest listed Bayer source, 16.1 KB at most, none without a
// Bayer source) and at most 80 registers: six workgroups a CU without a Bayer source, five with one of 640 columns, four from
// 880 columns on.  At the width cap a pass forms two output rows from four grey rows, a sub-pass one or two of those from four raw rows.
__global__ void __launch_bounds__(kConvThreads, 6) k_raw_linear(const ConvArgs A, const int32_t* __restrict__ list, int raw_lds) {
  __shared__ ConvShared sh;
  __shared__ RawRows rows;
  extern __shared__ __attribute__((aligned(16))) uint8_t raw_dyn[];
  const int li = blockIdx.x / A.bands;
  conv_linear<true>(sh, A, list[li], blockIdx.x - li * A.bands, RawStage{&rows, raw_dyn, raw_lds});
}

// k_convert_area: SL2_RESIZE_AREA.  A workgroup owns one sequence of the area list and a band of kConvBandRows output rows, and
// streams the band's source rows ONCE, from the first row tap to the last, through the same LDS staging (conv_stage: 16-byte
// loads, scalar head and tail) in passes of as many rows as the LDS holds (four at the width cap, sixteen at most).  Only a
// source row that straddles two bands is read by both.  The sum is separable and exact in any order, so the vertical pass comes
// first: for the output row at hand every lane owns source columns and adds wy g over the staged rows of that output row into
// colsum[x] (32 bits: at most 255 Sy), conflict-free byte reads of LDS with a uniform weight per row; a source row that
// straddles two output rows is read for both with its two weights, an output row that straddles two passes keeps its colsum.
// Once the output row's last source row has been staged a lane forms one output from colsum - a loop over the footprint: first
// and last column with their weights, D times the sum between -, in 32 bits, or 64 where 511 Sx Sy does not fit (decided per
// sequence), and rounds; every fourth lane gathers its three neighbours' bytes and stores four.  So the horizontal pass runs once per OUTPUT row, not per source row.
// Nothing is shared between workgroups: no atomics, no order.  Outputs wider than 1024 go through in panels of 1024 columns,
// each staging only the source columns its taps name.
// Budget: 16.5 KB of static LDS (the linear kernel's ConvShared) plus colsum, 4 bytes per source column of the widest AREA
// source (dynamic: 7.7 KB at 1920, 16.4 KB at the cap), and at most 80 registers: six workgroups a CU up to 2400 columns, four
// at the cap.  Compiled: 73 registers, no scratch.  (At the linear kernel's bound of 64 registers it spilled to scratch.)
struct AreaArgs {
  const sl2_frame_source* src;   // [nseq of the converter]
  const int32_t* list;           // the sequences whose filter is SL2_RESIZE_AREA
  const uint8_t* raw;
  uint8_t* out;
  unsigned long long seq_stride;
  int out_w, out_h, bands;
};

constexpr int kAreaPanel = 4 * kConvThreads;      // output columns a panel forms: four per lane

// colsum[x] = (fresh ? 0 : colsum[x]) + sum_j wy[j] grey[off[j] + x] for R staged rows
template <int R>
__device__ __forceinline__ void area_vertical(const uint8_t* __restrict__ grey, uint32_t* __restrict__ colsum, const int (&off)[4],
                                              const uint32_t (&wy)[4], int Wp, bool fresh) {
  for (int x = threadIdx.x; x < Wp; x += kConvThreads) {
    uint32_t v = fresh ? 0u : colsum[x];
#pragma unroll
    for (int j = 0; j < R; ++j) v += wy[j] * grey[off[j] + x];
    colsum[x] = v;
  }
}

template <typename ACC, bool RAW>
__device__ __forceinline__ void area_band(ConvShared& sh, uint32_t* __restrict__ colsum, const AreaArgs& A, const sl2_frame_source& src, int fmt,
                                          uint8_t* __restrict__ out, int band0, int band_end, const RawStage& rs) {
  const int tid = threadIdx.x;
  const int W = src.width, H = src.height, pitch = src.pitch;
  const int bpp = convert_bpp(fmt);
  const uint32_t n = (uint32_t)W * (uint32_t)H;
  const int y_first = convert_area_first(H, A.out_h, band0), y_last = convert_area_last(H, A.out_h, band_end - 1);
  for (int p0 = 0; p0 < A.out_w; p0 += kAreaPanel) {
    const int p1 = p0 + kAreaPanel < A.out_w ? p0 + kAreaPanel : A.out_w;
    const int xs = convert_area_first(W, A.out_w, p0), xe = convert_area_last(W, A.out_w, p1 - 1);
    const int Wp = xe - xs + 1;                                                // source columns this panel's taps name
    const uint8_t* __restrict__ base = A.raw + src.offset + (size_t)xs * bpp;
    const int wpad = conv_row_pad(Wp);
    const int fit = kConvLdsBytes / wpad;                                      // rows the LDS holds: at least 4
    const int cap = fit < kConvSlots ? fit : kConvSlots;
    // this lane's output columns p0 + tid and p0 + 256 + tid: their taps, once for all rows (further columns, of outputs wider
    // than 512, are worked out again row by row)
    AreaCol col0 = {xs, xs, 0, 0}, col1 = {xs, xs, 0, 0};
    if (p0 + tid < p1) col0 = convert_area_col(W, A.out_w, p0 + tid);
    if (p0 + kConvThreads + tid < p1) col1 = convert_area_col(W, A.out_w, p0 + kConvThreads + tid);
    int cur = band0;                                                           // the output row at hand (uniform)
    for (int c0 = y_first; c0 <= y_last; c0 += cap) {
      const int nrows = y_last - c0 + 1 < cap ? y_last - c0 + 1 : cap;
      const int c1 = c0 + nrows - 1;
      if (tid < nrows) sh.row[tid] = c0 + tid;
      if (tid == 0) sh.nslots = nrows;
      __syncthreads();
      if (RAW) raw_stage(sh, rs, A.raw + src.offset, pitch, W, H, xs, Wp, wpad, fmt);
      else switch (fmt) {
        case SL2_PIX_GRAY8: conv_stage<SL2_PIX_GRAY8>(sh, sh.grey, base, pitch, Wp, wpad); break;
        case SL2_PIX_RGB24: conv_stage<SL2_PIX_RGB24>(sh, sh.grey, base, pitch, Wp, wpad); break;
        case SL2_PIX_BGR24: conv_stage<SL2_PIX_BGR24>(sh, sh.grey, base, pitch, Wp, wpad); break;
        case SL2_PIX_UYVY: conv_stage<SL2_PIX_UYVY>(sh, sh.grey, base, pitch, Wp, wpad); break;
        default: conv_stage<SL2_PIX_YUYV>(sh, sh.grey, base, pitch, Wp, wpad); break;
      }
      __syncthreads();
      while (cur < band_end) {
        const int fy = convert_area_first(H, A.out_h, cur), ly = convert_area_last(H, A.out_h, cur);
        if (fy > c1) break;
        const int ya = fy > c0 ? fy : c0, yb = ly < c1 ? ly : c1;
        // vertical: colsum[x] (+)= sum_y wy g[y][x] over the staged rows of this output row, four rows at a time (their LDS
        // offsets and weights are uniform and stay in scalars); column x stays with its lane
        for (int y0 = ya; y0 <= yb; y0 += 4) {
          const bool fresh = y0 == fy;                                         // nothing of this output row is in colsum yet
          int off[4];
          uint32_t wy[4];
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const int y = y0 + j <= yb ? y0 + j : yb, k = y - c0;
            off[j] = k * wpad + sh.shift[k];
            wy[j] = (uint32_t)convert_area_weight(H, A.out_h, cur, y);
          }
          switch (yb - y0 + 1 < 4 ? yb - y0 + 1 : 4) {
            case 1: area_vertical<1>(sh.grey, colsum, off, wy, Wp, fresh); break;
            case 2: area_vertical<2>(sh.grey, colsum, off, wy, Wp, fresh); break;
            case 3: area_vertical<3>(sh.grey, colsum, off, wy, Wp, fresh); break;
            default: area_vertical<4>(sh.grey, colsum, off, wy, Wp, fresh); break;
          }
        }
        if (ly > c1) break;                                                    // the next pass brings the rest of this output row
        __syncthreads();
        // horizontal: a lane forms ONE output of the row from colsum (neighbouring lanes, neighbouring footprints), four
        // neighbours are gathered into the lane whose column is a multiple of four, which stores them as one word
        for (int cb = p0; cb < p1; cb += kConvThreads) {
          const int dx = cb + tid;
          uint32_t px = 0;
          if (dx < p1) {
            const AreaCol col = cb == p0 ? col0 : cb == p0 + kConvThreads ? col1 : convert_area_col(W, A.out_w, dx);
            px = convert_area_round(convert_area_hsum<ACC>(colsum, xs, col, A.out_w), n);
          }
          const uint32_t b1 = __shfl_down(px, 1), b2 = __shfl_down(px, 2), b3 = __shfl_down(px, 3);
          if ((tid & 3) == 0 && dx < p1) {
            const uint32_t packed = px | (b1 << 8) | (b2 << 16) | (b3 << 24);
            uint8_t* op = out + (size_t)cur * A.out_w + dx;
            const int left = A.out_w - dx;
            if (left >= 4 && ((uintptr_t)op & 3) == 0) {
              *reinterpret_cast<uint32_t*>(op) = packed;
            } else {
              for (int i = 0; i < 4 && i < left; ++i) op[i] = (uint8_t)(packed >> (8 * i));
            }
          }
        }
        __syncthreads();                                                       // colsum is the next output row's from here
        ++cur;
      }
      __syncthreads();      // the next pass overwrites the slots
    }
  }
}

__global__ void __launch_bounds__(kConvThreads, 6) k_convert_area(const AreaArgs A) {
  __shared__ ConvShared sh;
  extern __shared__ uint32_t area_colsum[];      // one word per source column of a panel
  const int li = blockIdx.x / A.bands, band = blockIdx.x - li * A.bands;
  const int s = A.list[li];
  const sl2_frame_source src = A.src[s];
  // never listed (the host refuses such sources, and lists those of a deep grey or Bayer format for k_raw_area)
  if ((src.format & (kConvAreaBit | kConvRawBit)) != kConvAreaBit || src.width < A.out_w || src.height < A.out_h) return;
  const int fmt = src.format & (kConvAreaBit - 1);
  uint8_t* __restrict__ out = A.out + (size_t)s * A.seq_stride;
  const int band0 = band * kConvBandRows;
  const int band_end = band0 + kConvBandRows < A.out_h ? band0 + kConvBandRows : A.out_h;
  const RawStage none{nullptr, nullptr, 0};
  if (convert_area_wide(src.width, src.height)) area_band<uint64_t, false>(sh, area_colsum, A, src, fmt, out, band0, band_end, none);
  else area_band<uint32_t, false>(sh, area_colsum, A, src, fmt, out, band0, band_end, none);
}

// k_raw_area: the same for the listed sequences, those of a deep grey or Bayer format under SL2_RESIZE_AREA: area_band over
// raw_stage.  A Bayer band stages raw rows y_first - 1 .. y_last + 1 (reflected); an output wider than 1024 stages, per panel, the
// raw columns either side of the panel's own.  Dynamic LDS: colsum (colsum_bytes, a multiple of 16), then the raw stage.  At
// most 80 registers; with a 1280-column Bayer source 16.5 + 0.6 + 5 + 16.1 KB: four workgroups a CU, three at the width cap.
__global__ void __launch_bounds__(kConvThreads, 6) k_raw_area(const AreaArgs A, int colsum_bytes, int raw_lds) {
  __shared__ ConvShared sh;
  __shared__ RawRows rows;
  extern __shared__ __attribute__((aligned(16))) uint32_t raw_area_dyn[];
  const int li = blockIdx.x / A.bands, band = blockIdx.x - li * A.bands;
  const int s = A.list[li];
  const sl2_frame_source src = A.src[s];
  if ((src.format & (kConvAreaBit | kConvRawBit)) != (kConvAreaBit | kConvRawBit) || src.width < A.out_w || src.height < A.out_h) return;
  const int fmt = src.format & kConvFormatMask;
  uint8_t* __restrict__ out = A.out + (size_t)s * A.seq_stride;
  const int band0 = band * kConvBandRows;
  const int band_end = band0 + kConvBandRows < A.out_h ? band0 + kConvBandRows : A.out_h;
  const RawStage rs{&rows, reinterpret_cast<uint8_t*>(raw_area_dyn) + colsum_bytes, raw_lds};
  if (convert_area_wide(src.width, src.height)) area_band<uint64_t, true>(sh, raw_area_dyn, A, src, fmt, out, band0, band_end, rs);
  else area_band<uint32_t, true>(sh, raw_area_dyn, A, src, fmt, out, band0, band_end, rs);
}

static std::string seq_text(int seq, const char* what) {
  char buf[160];
  snprintf(buf, sizeof(buf), "sequence %d: %s", seq, what);
  return buf;
}

}  // namespace sl2

using namespace sl2;

// The opaque converter of the C ABI: the sources of its sequences, their tap tables on the device, a staging buffer for raw
// frames that arrive in host memory.
struct sl2_converter {
  int device = 0, nseq = 0, out_w = 0, out_h = 0;
  int col_taps = 0, tap_stride = 0;
  std::vector<sl2_frame_source> src;
  std::vector<uint8_t> have;
  std::vector<int32_t> filter;           // SL2_RESIZE_* of every sequence
  ConvPlan plan;                         // what sl2_convert_frames launches: converter_upload makes it
  int32_t* d_lists = nullptr;            // [nseq]: plan.list on the device
  std::vector<uint32_t> taps;            // host copy of one sequence's table while it is built
  // the lens remap: nseq map slots (d_map nullptr: empty), the slot of every sequence (-1: none)
  struct MapSlot { int width = 0, height = 0, xbits = 0; uint32_t* d_map = nullptr; };
  std::vector<MapSlot> slots;
  std::vector<int32_t> remap;
  RemapSlotDev* d_slots = nullptr;       // [nseq]
  int32_t* d_remap = nullptr;            // [nseq]
  sl2_frame_source* d_src = nullptr;
  uint32_t* d_taps = nullptr;
  uint8_t* stage = nullptr;              // raw frames from host memory land here (grown on demand)
  size_t stage_bytes = 0;
  hipEvent_t done = nullptr;             // the last conversion queued: sl2_converter_set_sources and a growing stage wait for it
  bool queued = false;
};

// an output size the converter and the host forms take
static bool out_size_ok(int w, int h) { return w >= 1 && h >= 1 && w <= kConvertMaxOut && h <= kConvertMaxOut; }

// sequences seq0 .. seq0 + nseq - 1 lie in the converter
static bool converter_has_range(const sl2_converter* c, int seq0, int nseq) { return seq0 >= 0 && nseq >= 0 && seq0 + nseq <= c->nseq; }

// Wait for the last conversion queued: it keeps the tables, filters, maps, lists and the stage it was queued with
static int converter_quiesce(sl2_converter* c) {
  if (c->queued) { SL2_HIP(hipEventSynchronize(c->done)); c->queued = false; }
  return SL2_OK;
}

extern "C" int sl2_converter_create(int device, int nseq, int out_width, int out_height, sl2_converter** out) {
  if (!out || nseq < 1 || !out_size_ok(out_width, out_height)) {
    set_error("sl2_converter_create: nseq >= 1 and an output size of 1 .. 4096 per axis are required");
    return SL2_ERR_INVALID;
  }
  *out = nullptr;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { set_error("no HIP device"); return SL2_ERR_NO_DEVICE; }
  if (device < 0 || device >= ndev) { set_error("sl2_converter_create: no such device"); return SL2_ERR_INVALID; }
  SL2_HIP(hipSetDevice(device));
  sl2_converter* c = new sl2_converter;
  c->device = device; c->nseq = nseq; c->out_w = out_width; c->out_h = out_height;
  c->col_taps = round_up(out_width, 4);
  c->tap_stride = round_up(c->col_taps + out_height, 4);      // every table starts on a 16-byte boundary
  c->src.resize(nseq); c->have.assign(nseq, 0); c->taps.assign(c->tap_stride, 0); c->filter.assign(nseq, SL2_RESIZE_LINEAR);
  c->slots.resize(nseq); c->remap.assign(nseq, -1);
  hipError_t e = hipMalloc(&c->d_src, (size_t)nseq * sizeof(sl2_frame_source));
  if (e == hipSuccess) e = hipMalloc(&c->d_lists, (size_t)nseq * sizeof(int32_t));
  if (e == hipSuccess) e = hipMalloc(&c->d_taps, (size_t)nseq * c->tap_stride * sizeof(uint32_t));
  if (e == hipSuccess) e = hipMemset(c->d_taps, 0, (size_t)nseq * c->tap_stride * sizeof(uint32_t));
  if (e == hipSuccess) e = hipMalloc(&c->d_slots, (size_t)nseq * sizeof(RemapSlotDev));
  if (e == hipSuccess) e = hipMemset(c->d_slots, 0, (size_t)nseq * sizeof(RemapSlotDev));
  if (e == hipSuccess) e = hipMalloc(&c->d_remap, (size_t)nseq * sizeof(int32_t));
  if (e == hipSuccess) e = hipMemset(c->d_remap, 0xff, (size_t)nseq * sizeof(int32_t));
  if (e == hipSuccess) e = hipEventCreateWithFlags(&c->done, hipEventDisableTiming);
  if (e != hipSuccess) {
    set_error(std::string("sl2_converter_create: ") + hipGetErrorString(e));
    sl2_converter_destroy(c);
    return SL2_ERR_HIP;
  }
  *out = c;
  return SL2_OK;
}

extern "C" void sl2_converter_destroy(sl2_converter* c) {
  if (!c) return;
  hipSetDevice(c->device);
  if (c->queued) hipEventSynchronize(c->done);
  if (c->done) hipEventDestroy(c->done);
  if (c->d_src) hipFree(c->d_src);
  if (c->d_taps) hipFree(c->d_taps);
  if (c->d_lists) hipFree(c->d_lists);
  if (c->stage) hipFree(c->stage);
  for (auto& m : c->slots) if (m.d_map) hipFree(m.d_map);
  if (c->d_slots) hipFree(c->d_slots);
  if (c->d_remap) hipFree(c->d_remap);
  delete c;
}

// The device copies of sequences seq0 .. seq0 + nseq - 1 (the route rides in the format word), the plan and its lists.  No
// conversion is queued when this runs.
static int converter_upload(sl2_converter* c, int seq0, int nseq) {
  std::vector<sl2_frame_source> dev;
  int first = -1;
  for (int s = seq0; s < seq0 + nseq; ++s) {
    if (!c->have[s]) {
      if (first >= 0) { SL2_HIP(hipMemcpy(c->d_src + first, dev.data(), dev.size() * sizeof(sl2_frame_source), hipMemcpyHostToDevice)); dev.clear(); first = -1; }
      continue;
    }
    if (first < 0) first = s;
    dev.push_back(c->src[s]);
    dev.back().format |= convert_route_bits(convert_route(true, c->filter[s], c->src[s].format, c->remap[s]));
  }
  if (first >= 0) SL2_HIP(hipMemcpy(c->d_src + first, dev.data(), dev.size() * sizeof(sl2_frame_source), hipMemcpyHostToDevice));
  if (nseq > 0) SL2_HIP(hipMemcpy(c->d_remap + seq0, c->remap.data() + seq0, (size_t)nseq * sizeof(int32_t), hipMemcpyHostToDevice));
  c->plan = convert_plan(c->nseq, c->have.data(), c->src.data(), c->filter.data(), c->remap.data(), c->out_h);
  const std::vector<int32_t>& list = c->plan.list;
  if (!list.empty()) SL2_HIP(hipMemcpy(c->d_lists, list.data(), list.size() * sizeof(int32_t), hipMemcpyHostToDevice));
  return SL2_OK;
}

extern "C" int sl2_converter_set_sources(sl2_converter* c, int seq0, int nseq, const sl2_frame_source* src) {
  if (!c || !src || !converter_has_range(c, seq0, nseq)) { set_error("sl2_converter_set_sources: bad arguments"); return SL2_ERR_INVALID; }
  for (int i = 0; i < nseq; ++i) {
    const char* why = convert_source_fault(src[i], 0, false);
    if (!why && c->filter[seq0 + i] == SL2_RESIZE_AREA) why = convert_area_fault(src[i], c->out_w, c->out_h);
    if (!why && c->remap[seq0 + i] >= 0 && (src[i].width != c->slots[c->remap[seq0 + i]].width || src[i].height != c->slots[c->remap[seq0 + i]].height))
      why = "its map is for another source size";
    if (why) { set_error("sl2_converter_set_sources: " + seq_text(seq0 + i, why)); return SL2_ERR_INVALID; }
  }
  if (nseq == 0) return SL2_OK;
  SL2_HIP(hipSetDevice(c->device));
  if (int rc = converter_quiesce(c)) return rc;      // a queued conversion keeps its tables
  for (int i = 0; i < nseq; ++i) {
    if (!convert_tap_table(src[i].width, src[i].height, c->out_w, c->out_h, c->taps.data(), c->taps.data() + c->col_taps)) {
      set_error("sl2_converter_set_sources: " + seq_text(seq0 + i, "a tap does not fit its packed form"));
      return SL2_ERR_INVALID;
    }
    SL2_HIP(hipMemcpy(c->d_taps + (size_t)(seq0 + i) * c->tap_stride, c->taps.data(), (size_t)c->tap_stride * sizeof(uint32_t), hipMemcpyHostToDevice));
    c->src[seq0 + i] = src[i];
    c->have[seq0 + i] = 1;
  }
  return converter_upload(c, seq0, nseq);
}

extern "C" int sl2_converter_set_filters(sl2_converter* c, int seq0, int nseq, const int32_t* filters) {
  if (!c || !filters) { set_error("sl2_converter_set_filters: bad arguments"); return SL2_ERR_INVALID; }
  if (!converter_has_range(c, seq0, nseq)) {
    set_error("sl2_converter_set_filters: " + seq_text(seq0 < 0 ? seq0 : c->nseq, "outside the converter"));
    return SL2_ERR_INVALID;
  }
  for (int i = 0; i < nseq; ++i) {
    const char* why = nullptr;
    if (filters[i] != SL2_RESIZE_LINEAR && filters[i] != SL2_RESIZE_AREA) why = "unknown resize filter";
    else if (filters[i] == SL2_RESIZE_AREA && c->have[seq0 + i]) why = convert_area_fault(c->src[seq0 + i], c->out_w, c->out_h);
    if (why) { set_error("sl2_converter_set_filters: " + seq_text(seq0 + i, why)); return SL2_ERR_INVALID; }
  }
  if (nseq == 0) return SL2_OK;
  SL2_HIP(hipSetDevice(c->device));
  if (int rc = converter_quiesce(c)) return rc;      // a queued conversion keeps its filters
  for (int i = 0; i < nseq; ++i) c->filter[seq0 + i] = filters[i];
  return converter_upload(c, seq0, nseq);
}

extern "C" int sl2_converter_get_filters(const sl2_converter* c, int seq0, int nseq, int32_t* filters) {
  if (!c || !filters || !converter_has_range(c, seq0, nseq)) { set_error("sl2_converter_get_filters: bad arguments"); return SL2_ERR_INVALID; }
  for (int i = 0; i < nseq; ++i) filters[i] = c->filter[seq0 + i];
  return SL2_OK;
}

extern "C" int sl2_converter_get_sources(const sl2_converter* c, int seq0, int nseq, sl2_frame_source* src) {
  if (!c || !src || !converter_has_range(c, seq0, nseq)) { set_error("sl2_converter_get_sources: bad arguments"); return SL2_ERR_INVALID; }
  for (int i = 0; i < nseq; ++i) {
    if (!c->have[seq0 + i]) { set_error("sl2_converter_get_sources: " + seq_text(seq0 + i, "its source was never set")); return SL2_ERR_INVALID; }
    src[i] = c->src[seq0 + i];
  }
  return SL2_OK;
}

extern "C" int sl2_convert_frames(sl2_converter* c, void* stream, const void* raw, size_t raw_bytes, int raw_on_device,
                                  uint8_t* d_frames, size_t seq_stride) {
  if (!c || !raw || !d_frames) { set_error("sl2_convert_frames: bad arguments"); return SL2_ERR_INVALID; }
  if (seq_stride < (size_t)c->out_w * c->out_h) { set_error("sl2_convert_frames: seq_stride is below out_width * out_height"); return SL2_ERR_INVALID; }
  for (int s = 0; s < c->nseq; ++s) {
    if (!c->have[s]) { set_error("sl2_convert_frames: " + seq_text(s, "its source was never set")); return SL2_ERR_INVALID; }
    const char* why = convert_source_fault(c->src[s], raw_bytes, true);
    if (!why && raw_on_device && convert_is_deep(c->src[s].format) && ((uintptr_t)raw & 1)) why = "odd address of the raw buffer with a 16-bit format";
    if (why) { set_error("sl2_convert_frames: " + seq_text(s, why)); return SL2_ERR_INVALID; }
  }
  SL2_HIP(hipSetDevice(c->device));
  hipStream_t st = (hipStream_t)stream;
  const uint8_t* d_raw = (const uint8_t*)raw;
  if (!raw_on_device) {
    if (raw_bytes > c->stage_bytes) {
      if (int rc = converter_quiesce(c)) return rc;      // a queued conversion may still read the old one
      if (c->stage) { SL2_HIP(hipFree(c->stage)); c->stage = nullptr; c->stage_bytes = 0; }
      SL2_HIP(hipMalloc(&c->stage, raw_bytes));
      c->stage_bytes = raw_bytes;
    }
    SL2_HIP(hipMemcpyAsync(c->stage, raw, raw_bytes, hipMemcpyHostToDevice, st));
    d_raw = c->stage;
  }
  // a kernel per route that has a sequence: one launch for the reference's webcam, five at most.  The plan says which, on which
  // part of the lists and with how much dynamic LDS.
  const ConvPlan& P = c->plan;
  const auto grid = [&P](ConvRoute r) { return dim3((unsigned)(P.bands * P.count[r])); };
  const auto list = [&P, c](ConvRoute r) { return (const int32_t*)(c->d_lists + P.start[r]); };
  ConvArgs A;
  A.src = c->d_src; A.taps = c->d_taps; A.raw = d_raw; A.out = d_frames; A.seq_stride = seq_stride;
  A.out_w = c->out_w; A.out_h = c->out_h; A.col_taps = c->col_taps; A.tap_stride = c->tap_stride;
  A.bands = P.bands;
  // (k_convert_frames walks EVERY sequence and leaves the listed ones)
  if (P.count[kRouteLinear]) hipLaunchKernelGGL(k_convert_frames, dim3((unsigned)(P.bands * c->nseq)), dim3(kConvThreads), 0, st, A);
  AreaArgs B;
  B.src = c->d_src; B.list = list(kRouteArea); B.raw = d_raw; B.out = d_frames; B.seq_stride = seq_stride;
  B.out_w = c->out_w; B.out_h = c->out_h; B.bands = P.bands;
  if (P.count[kRouteArea]) hipLaunchKernelGGL(k_convert_area, grid(kRouteArea), dim3(kConvThreads), (size_t)P.lds[kRouteArea], st, B);
  if (P.count[kRouteRawLinear])
    hipLaunchKernelGGL(k_raw_linear, grid(kRouteRawLinear), dim3(kConvThreads), (size_t)P.lds[kRouteRawLinear], st, A, list(kRouteRawLinear),
                       P.lds[kRouteRawLinear]);
  if (P.count[kRouteRawArea]) {
    B.list = list(kRouteRawArea);
    hipLaunchKernelGGL(k_raw_area, grid(kRouteRawArea), dim3(kConvThreads), (size_t)P.lds[kRouteRawArea], st, B, P.raw_area_colsum,
                       P.lds[kRouteRawArea] - P.raw_area_colsum);
  }
  if (P.count[kRouteRemap]) {
    RemapArgs R;
    R.src = c->d_src; R.list = list(kRouteRemap); R.slot_of = c->d_remap; R.slots = c->d_slots;
    R.raw = d_raw; R.out = d_frames; R.seq_stride = seq_stride; R.out_w = c->out_w; R.out_h = c->out_h; R.bands = P.bands;
    convert_remap_launch(R, P.count[kRouteRemap], st);
  }
  SL2_HIP(hipGetLastError());
  SL2_HIP(hipEventRecord(c->done, st));
  c->queued = true;
  return SL2_OK;
}

extern "C" int sl2_convert_frame_host(const sl2_frame_source* src, const void* raw, size_t raw_bytes, int out_width, int out_height,
                                      uint8_t* out) {
  if (!src || !raw || !out || !out_size_ok(out_width, out_height)) {
    set_error("sl2_convert_frame_host: bad arguments");
    return SL2_ERR_INVALID;
  }
  const char* why = convert_source_fault(*src, raw_bytes, true);
  if (why) { set_error("sl2_convert_frame_host: " + seq_text(0, why)); return SL2_ERR_INVALID; }
  std::vector<uint32_t> taps((size_t)out_width + out_height);
  if (!convert_frame_host_body(*src, (const uint8_t*)raw, out_width, out_height, taps.data(), taps.data() + out_width, out)) {
    set_error("sl2_convert_frame_host: a tap does not fit its packed form");
    return SL2_ERR_INVALID;
  }
  return SL2_OK;
}

extern "C" int sl2_convert_frame_host_filtered(const sl2_frame_source* src, int filter, const void* raw, size_t raw_bytes, int out_width,
                                               int out_height, uint8_t* out) {
  if (filter == SL2_RESIZE_LINEAR) return sl2_convert_frame_host(src, raw, raw_bytes, out_width, out_height, out);
  if (filter != SL2_RESIZE_AREA) { set_error("sl2_convert_frame_host_filtered: unknown resize filter"); return SL2_ERR_INVALID; }
  if (!src || !raw || !out || !out_size_ok(out_width, out_height)) {
    set_error("sl2_convert_frame_host_filtered: bad arguments");
    return SL2_ERR_INVALID;
  }
  const char* why = convert_source_fault(*src, raw_bytes, true);
  if (!why) why = convert_area_fault(*src, out_width, out_height);
  if (why) { set_error("sl2_convert_frame_host_filtered: " + seq_text(0, why)); return SL2_ERR_INVALID; }
  std::vector<uint8_t> grey((size_t)src->width);
  std::vector<AreaCol> cols((size_t)out_width);
  std::vector<uint64_t> acc((size_t)out_width);
  convert_frame_host_area_body(*src, (const uint8_t*)raw, out_width, out_height, grey.data(), cols.data(), acc.data(), out);
  return SL2_OK;
}

extern "C" int sl2_scale_camera(const sl2_camera* in, int out_width, int out_height, sl2_camera* out) {
  if (!in || !out || in->width < 1 || in->height < 1 || out_width < 1 || out_height < 1) { set_error("sl2_scale_camera: bad arguments"); return SL2_ERR_INVALID; }
  if ((long long)in->width * out_height != (long long)in->height * out_width) {
    set_error("sl2_scale_camera: the resize changes the aspect ratio; the radial distortion term survives a uniform scale only");
    return SL2_ERR_INVALID;
  }
  const double s = (double)in->width / (double)out_width;
  sl2_camera r = *in;
  r.width = out_width; r.height = out_height;
  r.fku = in->fku / s; r.fkv = in->fkv / s;
  r.u0 = (in->u0 + 0.5) / s - 0.5; r.v0 = (in->v0 + 0.5) / s - 0.5;
  r.kd1 = in->kd1 * s * s;
  *out = r;
  return SL2_OK;
}

// ---- the lens remap

// The first sequence that follows `slot`, -1: none
static int converter_slot_user(const sl2_converter* c, int slot) {
  for (int s = 0; s < c->nseq; ++s) if (c->remap[s] == slot) return s;
  return -1;
}

extern "C" int sl2_converter_set_map(sl2_converter* c, int slot, int src_width, int src_height, const int32_t* xy) {
  if (!c) { set_error("sl2_converter_set_map: bad arguments"); return SL2_ERR_INVALID; }
  if (slot < 0 || slot >= c->nseq) { set_error("sl2_converter_set_map: slot outside 0 .. nseq - 1"); return SL2_ERR_INVALID; }
  sl2_converter::MapSlot& m = c->slots[slot];
  const int user = converter_slot_user(c, slot);
  if (!xy) {
    if (user >= 0) { set_error("sl2_converter_set_map: " + seq_text(user, "still uses the slot that would be emptied")); return SL2_ERR_INVALID; }
  } else {
    if (src_width < 1 || src_height < 1 || src_width > kConvertMaxWidth || src_height > kConvertMaxHeight) {
      set_error("sl2_converter_set_map: a source size of 1 .. 4096 by 1 .. 16384 is required");
      return SL2_ERR_INVALID;
    }
    if (user >= 0 && (src_width != m.width || src_height != m.height)) {
      set_error("sl2_converter_set_map: " + seq_text(user, "still uses the slot, whose source size would change"));
      return SL2_ERR_INVALID;
    }
  }
  SL2_HIP(hipSetDevice(c->device));
  if (int rc = converter_quiesce(c)) return rc;      // a queued conversion keeps its map
  RemapSlotDev dev = {nullptr, 0, 0, 0, 0};
  if (!xy) {
    if (m.d_map) { SL2_HIP(hipFree(m.d_map)); }
    m = sl2_converter::MapSlot();
  } else {
    // the device form: entries that reach no source pixel become the border, the rest one word each where the size allows
    const size_t n = (size_t)c->out_w * (size_t)c->out_h;
    const int xbits = remap_packed_xbits(src_width, src_height);
    std::vector<uint32_t> words(xbits ? n : 2 * n);
    for (size_t i = 0; i < n; ++i) {
      const int32_t X = xy[2 * i], Y = xy[2 * i + 1];
      const bool live = remap_reaches(src_width, src_height, X, Y);
      if (xbits) words[i] = live ? remap_pack(xbits, X, Y) : kRemapBorderWord;
      else { words[2 * i] = (uint32_t)(live ? X : SL2_REMAP_BORDER); words[2 * i + 1] = live ? (uint32_t)Y : 0u; }
    }
    uint32_t* d_new = nullptr;
    SL2_HIP(hipMalloc(&d_new, words.size() * sizeof(uint32_t)));
    hipError_t e = hipMemcpy(d_new, words.data(), words.size() * sizeof(uint32_t), hipMemcpyHostToDevice);
    if (e != hipSuccess) { hipFree(d_new); set_error(std::string("sl2_converter_set_map: ") + hipGetErrorString(e)); return SL2_ERR_HIP; }
    if (m.d_map) { SL2_HIP(hipFree(m.d_map)); }
    m.d_map = d_new; m.width = src_width; m.height = src_height; m.xbits = xbits;
    dev.map = d_new; dev.width = src_width; dev.height = src_height; dev.xbits = xbits;
  }
  SL2_HIP(hipMemcpy(c->d_slots + slot, &dev, sizeof(dev), hipMemcpyHostToDevice));
  return SL2_OK;
}

extern "C" int sl2_converter_set_remaps(sl2_converter* c, int seq0, int nseq, const int32_t* slots) {
  if (!c || !slots) { set_error("sl2_converter_set_remaps: bad arguments"); return SL2_ERR_INVALID; }
  if (!converter_has_range(c, seq0, nseq)) {
    set_error("sl2_converter_set_remaps: " + seq_text(seq0 < 0 ? seq0 : c->nseq, "outside the converter"));
    return SL2_ERR_INVALID;
  }
  for (int i = 0; i < nseq; ++i) {
    const char* why = nullptr;
    const int k = slots[i];
    if (k < -1 || k >= c->nseq) why = "slot outside -1 .. nseq - 1";
    else if (k >= 0 && !c->slots[k].d_map) why = "its map slot is empty";
    else if (k >= 0 && c->have[seq0 + i] && (c->src[seq0 + i].width != c->slots[k].width || c->src[seq0 + i].height != c->slots[k].height))
      why = "its source has another size than the map's";
    if (why) { set_error("sl2_converter_set_remaps: " + seq_text(seq0 + i, why)); return SL2_ERR_INVALID; }
  }
  if (nseq == 0) return SL2_OK;
  SL2_HIP(hipSetDevice(c->device));
  if (int rc = converter_quiesce(c)) return rc;      // a queued conversion keeps its lists
  for (int i = 0; i < nseq; ++i) c->remap[seq0 + i] = slots[i];
  return converter_upload(c, seq0, nseq);
}

extern "C" int sl2_converter_get_remaps(const sl2_converter* c, int seq0, int nseq, int32_t* slots) {
  if (!c || !slots || !converter_has_range(c, seq0, nseq)) { set_error("sl2_converter_get_remaps: bad arguments"); return SL2_ERR_INVALID; }
  for (int i = 0; i < nseq; ++i) slots[i] = c->remap[seq0 + i];
  return SL2_OK;
}

extern "C" int sl2_remap_frame_host(const sl2_frame_source* src, const int32_t* xy, const void* raw, size_t raw_bytes, int out_width,
                                    int out_height, uint8_t* out) {
  if (!src || !xy || !raw || !out || !out_size_ok(out_width, out_height)) {
    set_error("sl2_remap_frame_host: bad arguments");
    return SL2_ERR_INVALID;
  }
  const char* why = convert_source_fault(*src, raw_bytes, true);
  if (why) { set_error("sl2_remap_frame_host: " + seq_text(0, why)); return SL2_ERR_INVALID; }
  remap_frame_host_body(*src, xy, (const uint8_t*)raw, out_width, out_height, out);
  return SL2_OK;
}

static const char* lens_fault(const sl2_lens& l) {
  if (l.model != SL2_LENS_RADIAL1 && l.model != SL2_LENS_BROWN && l.model != SL2_LENS_FISHEYE) return "unknown lens model";
  if (l.width < 1 || l.height < 1 || l.width > kConvertMaxWidth || l.height > kConvertMaxHeight) return "a lens image of 1 .. 4096 by 1 .. 16384 is required";
  return nullptr;
}

extern "C" int sl2_lens_map_host(const sl2_lens* lens, const sl2_camera* target, int32_t* xy) {
  if (!lens || !target || !xy) { set_error("sl2_lens_map_host: bad arguments"); return SL2_ERR_INVALID; }
  const char* why = lens_fault(*lens);
  if (!why && !out_size_ok(target->width, target->height))
    why = "a target size of 1 .. 4096 per axis is required";
  if (why) { set_error(std::string("sl2_lens_map_host: ") + why); return SL2_ERR_INVALID; }
  for (int y = 0; y < target->height; ++y)
    for (int x = 0; x < target->width; ++x) {
      int32_t* e = xy + 2 * ((size_t)y * target->width + x);
      lens_map_entry(*lens, *target, x, y, &e[0], &e[1]);
    }
  return SL2_OK;
}

extern "C" int sl2_lens_pinhole_camera(const sl2_lens* lens, int out_width, int out_height, int sd, sl2_camera* out) {
  if (!lens || !out) { set_error("sl2_lens_pinhole_camera: bad arguments"); return SL2_ERR_INVALID; }
  const char* why = lens_fault(*lens);
  if (!why && !out_size_ok(out_width, out_height)) why = "an output size of 1 .. 4096 per axis is required";
  if (why) { set_error(std::string("sl2_lens_pinhole_camera: ") + why); return SL2_ERR_INVALID; }
  sl2_camera r;
  r.width = out_width; r.height = out_height;
  r.fku = lens->fx * (double)out_width / (double)lens->width;
  r.fkv = lens->fy * (double)out_height / (double)lens->height;
  r.u0 = (lens->cx + 0.5) * (double)out_width / (double)lens->width - 0.5;
  r.v0 = (lens->cy + 0.5) * (double)out_height / (double)lens->height - 0.5;
  r.kd1 = 0.0; r.sd = sd;
  *out = r;
  return SL2_OK;
}
