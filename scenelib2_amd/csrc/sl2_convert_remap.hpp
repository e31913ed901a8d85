// The lens remap's kernel lives in a unit of its own (sl2_convert_remap.hip): what that unit and the converter's host code
// (sl2_convert.hip) share, beside the constants and the route bits of sl2_convert_plan.hpp.  The arithmetic is
// sl2_convert_dev.hpp's remap_pixel.
#pragma once
#include "sl2_common.hpp"
#include "sl2_convert_plan.hpp"

namespace sl2 {

struct RemapSlotDev {            // 24 bytes
  const uint32_t* map;           // [out_h][out_w] words (xbits > 0) or [out_h][out_w][2] (xbits == 0); nullptr: an empty slot
  int32_t width, height;         // the source size the map is for
  int32_t xbits, pad;            // remap_packed_xbits
};
struct RemapArgs {
  const sl2_frame_source* src;   // [nseq of the converter]
  const int32_t* list;           // the sequences that follow a map
  const int32_t* slot_of;        // [nseq]: the slot of every sequence (-1: none)
  const RemapSlotDev* slots;     // [nseq]
  const uint8_t* raw;
  uint8_t* out;
  unsigned long long seq_stride;
  int out_w, out_h, bands;
};

// One launch for `nlisted` sequences of A.list on `stream`
void convert_remap_launch(const RemapArgs& A, int nlisted, hipStream_t stream);

}  // namespace sl2
