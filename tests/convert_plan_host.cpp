// Stand-alone host build of the frame converter's plan (scenelib2_amd/csrc/sl2_convert_plan.hpp, no HIP): what
// tests/test_convert_plan_host.py asks of it.  The test compiles it with -fsanitize=address,undefined and runs it; nothing is
// loaded into Python.
// in (the file named on the command line): the number of cases; per case "nseq out_h", then per sequence
// "have width format filter remap_slot".
// out: a line of constants, a line with convert_route_bits of the five routes, then per case the plan member by member, each
// sequence's route and the bits of its device record, and the list.
#include <cstdio>
#include <vector>

#include "../scenelib2_amd/csrc/sl2_convert_plan.hpp"

using namespace sl2;

static void print_ints(const char* name, const int* v, int n) {
  printf("%s", name);
  for (int i = 0; i < n; ++i) printf(" %d", v[i]);
  printf("\n");
}

int main(int argc, char** argv) {
  FILE* f = argc == 2 ? fopen(argv[1], "r") : nullptr;
  if (!f) { fprintf(stderr, "usage: convert_plan_host CASES\n"); return 2; }
  const int constants[] = {kConvThreads, kConvBandRows, kConvSlots, kConvLdsBytes, kRawSlots, kRawLdsBytes, kConvAreaBit, kConvRawBit,
                           kConvRemapBit, kConvFormatMask, conv_row_pad(1), conv_row_pad(2), conv_row_pad(3), conv_row_pad(4096)};
  print_ints("constants", constants, (int)(sizeof(constants) / sizeof(constants[0])));
  const int route_bits[] = {convert_route_bits(kRouteNone), convert_route_bits(kRouteLinear), convert_route_bits(kRouteArea),
                            convert_route_bits(kRouteRawLinear), convert_route_bits(kRouteRawArea), convert_route_bits(kRouteRemap)};
  print_ints("route_bits", route_bits, 6);
  int ncases = 0;
  if (fscanf(f, "%d", &ncases) != 1) return 2;
  for (int k = 0; k < ncases; ++k) {
    int nseq = 0, out_h = 0;
    if (fscanf(f, "%d %d", &nseq, &out_h) != 2 || nseq < 1) return 2;
    std::vector<uint8_t> have(nseq);
    std::vector<sl2_frame_source> src(nseq);
    std::vector<int32_t> filter(nseq), remap(nseq);
    for (int s = 0; s < nseq; ++s) {
      int h, w, fmt, flt, slot;
      if (fscanf(f, "%d %d %d %d %d", &h, &w, &fmt, &flt, &slot) != 5) return 2;
      have[s] = (uint8_t)h; filter[s] = flt; remap[s] = slot;
      src[s] = sl2_frame_source();
      src[s].width = w; src[s].height = 1; src[s].format = fmt;
    }
    const ConvPlan p = convert_plan(nseq, have.data(), src.data(), filter.data(), remap.data(), out_h);
    printf("case %d\n", k);
    print_ints("count", p.count, kConvRoutes);
    print_ints("start", p.start, kConvRoutes);
    print_ints("lds", p.lds, kConvRoutes);
    print_ints("colsum", &p.raw_area_colsum, 1);
    print_ints("bands", &p.bands, 1);
    std::vector<int> route(nseq), bits(nseq);
    for (int s = 0; s < nseq; ++s) {
      const ConvRoute r = convert_route(have[s] != 0, filter[s], src[s].format, remap[s]);
      route[s] = (int)r; bits[s] = convert_route_bits(r);
    }
    print_ints("route", route.data(), nseq);
    print_ints("bits", bits.data(), nseq);
    print_ints("list", p.list.data(), (int)p.list.size());
  }
  fclose(f);
  printf("ok %d cases\n", ncases);
  return 0;
}
