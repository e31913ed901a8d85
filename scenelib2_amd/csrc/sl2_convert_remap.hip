// The lens remap's kernel ("the lens remap"; the arithmetic: sl2_convert_dev.hpp, remap_pixel; the converter
// that launches it: sl2_convert.hip; which sequences it is launched for: sl2_convert_plan.hpp, kRouteRemap).  A unit of its own:
// the device code of the converter's other four kernels is, byte for byte, what it was before this kernel existed.
#include "sl2_convert_remap.hpp"

namespace sl2 {

// k_convert_remap: the lens remap (sl2_convert_dev.hpp, remap_pixel).  A workgroup owns one sequence of the remap list and a band of
// kConvBandRows output rows.  The band's map entries and its outputs are ONE run of rows x out_w consecutive elements each (the
// rows follow each other without a gap), so the kernel has no rows or columns of its own: a wave takes 256 consecutive elements at
// a time, lane l those at l, l + 64, l + 128 and l + 192.  Every load or store instruction of a wave then covers 64 NEIGHBOURING
// outputs: the map entries are one coalesced run, and the taps of neighbouring outputs are neighbours in the source, so a gather
// instruction touches the two or three 128-byte lines under them - with four consecutive outputs per lane (the siblings' shape) it
// touched four to eight, and was 1.2 to 2.1 times slower.  The taps come straight from the raw buffer through remap_pixel itself,
// so the bytes are the host form's by construction.  Nothing is staged in LDS: where a map bends, the source rows of a band are
// not known before the map is read.  A tap counts only where it lies in the image and has a weight above 0, and the bytes fetched
// for the others come from clamped, in-image coordinates (remap_pixel has no branch: the loads of a lane's four outputs are in
// flight at once, not one behind the other); Bayer neighbours are reflected in the index: nothing outside the source is ever
// addressed.  Budget: no LDS, at most 80 registers, six waves a SIMD.  (At the linear kernel's bound of 64 the 4 x 4 Bayer bytes of a
// lane's four outputs spilled to scratch.)
__global__ void __launch_bounds__(kConvThreads, 6) k_convert_remap(const RemapArgs A) {
  const int li = blockIdx.x / A.bands, band = blockIdx.x - li * A.bands;
  const int s = A.list[li];
  const int si = A.slot_of[s];
  const sl2_frame_source src = A.src[s];
  if (si < 0 || !(src.format & kConvRemapBit)) return;      // never listed
  const RemapSlotDev slot = A.slots[si];
  if (!slot.map || slot.width != src.width || slot.height != src.height) return;      // never listed (the host refuses both)
  const int fmt = src.format & kConvFormatMask, W = src.width, H = src.height, pitch = src.pitch, xbits = slot.xbits;
  const uint8_t* __restrict__ base = A.raw + src.offset;
  const int band0 = band * kConvBandRows;
  const int band_end = band0 + kConvBandRows < A.out_h ? band0 + kConvBandRows : A.out_h;
  const size_t e0 = (size_t)band0 * (size_t)A.out_w;                           // the band's first element
  const int n = (band_end - band0) * A.out_w;                                  // its elements: at most 8 x 4096
  const uint32_t* __restrict__ map1 = slot.map + e0;                           // one-word entries ...
  const uint2* __restrict__ map2 = reinterpret_cast<const uint2*>(slot.map) + e0;      // ... or two-word ones (8-byte aligned: hipMalloc)
  uint8_t* __restrict__ out = A.out + (size_t)s * A.seq_stride + e0;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int k0 = wave * 256; k0 < n; k0 += kConvThreads * 4) {
    int32_t X[4], Y[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int k = k0 + 64 * i + lane;
      X[i] = SL2_REMAP_BORDER; Y[i] = 0;                                       // past the band: a border entry, not stored
      if (k < n) {
        if (xbits) remap_unpack(xbits, map1[k], &X[i], &Y[i]);
        else { const uint2 w = map2[k]; X[i] = (int32_t)w.x; Y[i] = (int32_t)w.y; }
      }
    }
    uint8_t px[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) px[i] = remap_pixel(fmt, base, pitch, W, H, X[i], Y[i]);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int k = k0 + 64 * i + lane;
      if (k < n) out[k] = px[i];
    }
  }
}

void convert_remap_launch(const RemapArgs& A, int nlisted, hipStream_t stream) {
  hipLaunchKernelGGL(k_convert_remap, dim3((unsigned)(A.bands * nlisted)), dim3(kConvThreads), 0, stream, A);
}

}  // namespace sl2
