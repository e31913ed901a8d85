// Host build of the per-sequence camera record's constants (sl2_common.hpp, the HIP headers in host mode): what
// tests/test_seq_camera_host.py asks of them.
#include "../scenelib2_amd/csrc/sl2_common.hpp"

using namespace sl2;

static_assert(kSeqCamDoubles == 8 && kSeqCamDoubles * sizeof(double) == 64, "one 64-byte line per sequence");
static_assert(kSeqCamFku == 0 && kSeqCamFkv == 1 && kSeqCamU0 == 2 && kSeqCamV0 == 3 && kSeqCamKd1 == 4 && kSeqCamSd == 5, "the places");
static_assert(kSeqCamSd < kSeqCamDoubles - 2, "two spare words behind the six intrinsics");

extern "C" {
int sc_record_bytes() { return (int)(kSeqCamDoubles * sizeof(double)); }
int sc_camera_bytes() { return (int)sizeof(sl2_camera); }
int sc_blob_header_bytes() { return (int)sizeof(sl2_sequence_blob_header); }
}
