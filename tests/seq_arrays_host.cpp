// Host build of the table of per-sequence arrays (sl2_seq_arrays.hpp, no HIP): what tests/test_seq_arrays_host.py asks of it.
#include "../scenelib2_amd/csrc/sl2_seq_arrays.hpp"

using namespace sl2;

namespace {
struct Row { const char* name; size_t elem_size; };
#define X(type, name, elems) {#name, sizeof(type)},
const Row kRows[] = {SL2_SEQ_ARRAYS(X)};
#undef X
const int kCount = (int)(sizeof(kRows) / sizeof(kRows[0]));
}  // namespace

extern "C" {

int sa_count() { return kCount; }
// the members of SeqArrays are the rows and nothing else: one pointer each
int sa_struct_pointers() { return (int)(sizeof(SeqArrays) / sizeof(void*)); }
const char* sa_name(int i) { return i >= 0 && i < kCount ? kRows[i].name : nullptr; }
size_t sa_elem_size(int i) { return i >= 0 && i < kCount ? kRows[i].elem_size : 0; }

// elements per sequence of row i
size_t sa_elems(int i, size_t N, size_t ld, size_t mld, size_t nblk_max, size_t kpart, size_t pcap) {
#define X(type, name, elems) (size_t)(elems),
  const size_t all[] = {SL2_SEQ_ARRAYS(X)};
#undef X
  return i >= 0 && i < kCount ? all[i] : 0;
}

// bytes by which seq_arrays_view advances row i for a group that starts at sequence `first`
size_t sa_view_offset(int i, size_t N, size_t ld, size_t mld, size_t nblk_max, size_t kpart, size_t pcap, size_t first) {
  SeqArrays root;
  char* const base = reinterpret_cast<char*>((uintptr_t)1 << 40);
#define X(type, name, elems) root.name = reinterpret_cast<type*>(base);
  SL2_SEQ_ARRAYS(X)
#undef X
  const SeqArrays v = seq_arrays_view(root, SeqDims{N, ld, mld, nblk_max, kpart, pcap}, first);
#define X(type, name, elems) (size_t)(reinterpret_cast<const char*>(v.name) - base),
  const size_t all[] = {SL2_SEQ_ARRAYS(X)};
#undef X
  return i >= 0 && i < kCount ? all[i] : 0;
}

void sa_group_range(int B, int G, int k, int* first, int* count) { group_range(B, G, k, first, count); }

}  // extern "C"
