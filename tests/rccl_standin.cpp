// A test-only stand-in for the ten RCCL calls scenelib2_amd/csrc/sl2_comm.hip makes, so that the library's own multi-rank
// code (block offsets, who skips an empty block, roots other than 0, the grouped form, stream ordering, row order of the
// gather) runs on ONE device: RCCL refuses two ranks of a clique on the same GPU, this does not.  Host C++ and the HIP runtime
// API only (device-to-device hipMemcpyAsync and events), no kernels.  Linked with the product's sl2_comm.o into
// scenelib2_amd/libscenelib2_amd_comm_test.so (csrc/Makefile); the signatures are checked against the real <rccl/rccl.h>.
//
// Semantics (tests/test_gpu_comm_multirank.py relies on them):
//  * group calls nest; operations are queued per host thread and posted at the outermost ncclGroupEnd, an operation outside
//    a group at once.  Posting puts them into one process-wide table; the posting thread executes whatever has thereby become
//    complete (a send and its receive; an all-gather every rank of the clique has posted), then waits until all of ITS
//    operations have been executed - by itself (one thread, grouped: nothing waits) or by a peer's thread (the rendezvous).
//  * the wait is bounded (kRendezvousSeconds): a mismatch fails a test with ncclInternalError, it does not hang it.
//  * stricter than RCCL where RCCL would hang or corrupt: different byte counts of a send / receive pair, different counts or
//    types in an all-gather, a peer out of range, a rank that joins a clique twice and an unbalanced ncclGroupEnd are
//    ncclInvalidArgument.
//  * stream order as with RCCL: the receiver's stream waits for what the sender's stream had queued, the copy runs on the
//    receiver's stream, the sender's stream waits for the copy (so it may reuse its buffer in stream order).
#include <rccl/rccl.h>

#include <hip/hip_runtime_api.h>

#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstring>
#include <map>
#include <mutex>
#include <string>
#include <vector>

namespace {

constexpr int kRendezvousSeconds = 20;   // bound of every wait for a peer

struct Clique {
  int nranks = 0;
  int live = 0;          // communicators created and not yet destroyed
  bool formed = false;   // every rank has joined
  std::vector<bool> joined;   // ncclCommInitRank: which ranks have arrived
};

}  // namespace

struct ncclComm {
  Clique* clique;
  int rank;
  int device;
};

namespace {

enum Kind { kSend, kRecv, kGather };

struct Op {
  Kind kind;
  ncclComm* comm;
  const void* src;
  void* dst;
  size_t count;
  ncclDataType_t type;
  int peer;
  hipStream_t stream;
  bool done = false;
  ncclResult_t result = ncclSuccess;
  const char* why = nullptr;   // what went wrong (static text)
};

std::mutex g_mu;
std::condition_variable g_cv;
std::vector<Op*> g_table;                   // posted and not yet executed, in posting order
std::map<std::string, Clique*> g_forming;   // ncclCommInitRank: cliques some ranks of which have yet to arrive
std::vector<hipEvent_t> g_spent;            // events a stream may still be waiting on: destroyed once they have completed
std::atomic<int> g_live{0};
std::atomic<unsigned long long> g_next_id{1};

thread_local int t_depth = 0;
thread_local std::vector<Op> t_queue;
thread_local ncclResult_t t_detail_code = ncclSuccess;
thread_local std::string t_detail;

ncclResult_t refuse(ncclResult_t code, const char* base, const char* why) {
  t_detail_code = code;
  t_detail = std::string(base) + " (stand-in: " + why + ")";
  return code;
}
ncclResult_t invalid(const char* why) { return refuse(ncclInvalidArgument, "invalid argument", why); }

size_t type_size(ncclDataType_t t) {
  switch (t) {
    case ncclInt8: case ncclUint8: return 1;
    case ncclFloat16: case ncclBfloat16: return 2;
    case ncclInt32: case ncclUint32: case ncclFloat32: return 4;
    case ncclInt64: case ncclUint64: case ncclFloat64: return 8;
    default: return 0;
  }
}

// ---- events (g_mu held) ----

void reap() {
  size_t k = 0;
  for (hipEvent_t ev : g_spent) {
    if (hipEventQuery(ev) == hipErrorNotReady) g_spent[k++] = ev;
    else (void)hipEventDestroy(ev);
  }
  g_spent.resize(k);
}

struct DeviceGuard {
  int saved = 0;
  DeviceGuard() { (void)hipGetDevice(&saved); }
  ~DeviceGuard() { (void)hipSetDevice(saved); }
};

#define STANDIN_HIP(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) return e_; } while (0)

hipError_t record_event(int dev, hipStream_t st, hipEvent_t* ev) {
  STANDIN_HIP(hipSetDevice(dev));
  STANDIN_HIP(hipEventCreateWithFlags(ev, hipEventDisableTiming));
  g_spent.push_back(*ev);
  STANDIN_HIP(hipEventRecord(*ev, st));
  return hipSuccess;
}

hipError_t wait_event(int dev, hipStream_t st, hipEvent_t ev) {
  STANDIN_HIP(hipSetDevice(dev));
  STANDIN_HIP(hipStreamWaitEvent(st, ev, 0));
  return hipSuccess;
}

bool same_queue(const Op* a, const Op* b) { return a->comm->device == b->comm->device && a->stream == b->stream; }

hipError_t run_pair(const Op* s, const Op* r, size_t bytes) {
  if (bytes == 0) return hipSuccess;
  const bool shared = same_queue(s, r);
  hipEvent_t ev;
  if (!shared) {
    STANDIN_HIP(record_event(s->comm->device, s->stream, &ev));
    STANDIN_HIP(wait_event(r->comm->device, r->stream, ev));
  }
  STANDIN_HIP(hipSetDevice(r->comm->device));
  STANDIN_HIP(hipMemcpyAsync(r->dst, s->src, bytes, hipMemcpyDeviceToDevice, r->stream));
  if (!shared) {
    STANDIN_HIP(record_event(r->comm->device, r->stream, &ev));
    STANDIN_HIP(wait_event(s->comm->device, s->stream, ev));
  }
  return hipSuccess;
}

hipError_t run_gather(const std::vector<Op*>& ops, size_t bytes) {   // ops[rank]
  if (bytes == 0) return hipSuccess;
  const int n = (int)ops.size();
  std::vector<hipEvent_t> filled(n), copied(n);
  for (int s = 0; s < n; ++s) STANDIN_HIP(record_event(ops[s]->comm->device, ops[s]->stream, &filled[s]));
  for (int d = 0; d < n; ++d) {
    for (int s = 0; s < n; ++s) {
      if (!same_queue(ops[s], ops[d])) STANDIN_HIP(wait_event(ops[d]->comm->device, ops[d]->stream, filled[s]));
      char* to = (char*)ops[d]->dst + (size_t)s * bytes;
      if ((const void*)to == ops[s]->src) continue;   // in place
      STANDIN_HIP(hipSetDevice(ops[d]->comm->device));
      STANDIN_HIP(hipMemcpyAsync(to, ops[s]->src, bytes, hipMemcpyDeviceToDevice, ops[d]->stream));
    }
    STANDIN_HIP(record_event(ops[d]->comm->device, ops[d]->stream, &copied[d]));
  }
  for (int s = 0; s < n; ++s)
    for (int d = 0; d < n; ++d)
      if (!same_queue(ops[s], ops[d])) STANDIN_HIP(wait_event(ops[s]->comm->device, ops[s]->stream, copied[d]));
  return hipSuccess;
}

// ---- the table (g_mu held) ----

void finish(Op* o, ncclResult_t result, const char* why) {
  o->result = result;
  o->why = why;
  o->done = true;
}

void take_out(Op* o) {
  for (size_t i = 0; i < g_table.size(); ++i)
    if (g_table[i] == o) { g_table.erase(g_table.begin() + i); return; }
}

bool match_one_pair() {
  for (Op* s : g_table) {
    if (s->kind != kSend) continue;
    for (Op* r : g_table) {
      if (r->kind != kRecv || r->comm->clique != s->comm->clique || r->comm->rank != s->peer || r->peer != s->comm->rank) continue;
      take_out(s);
      take_out(r);
      const size_t sb = s->count * type_size(s->type), rb = r->count * type_size(r->type);
      if (sb != rb) {
        finish(s, ncclInvalidArgument, "ncclSend and the matching ncclRecv differ in their byte counts");
        finish(r, ncclInvalidArgument, "ncclRecv and the matching ncclSend differ in their byte counts");
      } else {
        const hipError_t e = run_pair(s, r, sb);
        finish(s, e == hipSuccess ? ncclSuccess : ncclUnhandledCudaError, e == hipSuccess ? nullptr : hipGetErrorString(e));
        finish(r, s->result, s->why);
      }
      return true;
    }
  }
  return false;
}

bool match_one_gather() {
  for (Op* g : g_table) {
    if (g->kind != kGather) continue;
    Clique* K = g->comm->clique;
    std::vector<Op*> ops(K->nranks, nullptr);
    int have = 0;
    for (Op* o : g_table)
      if (o->kind == kGather && o->comm->clique == K && !ops[o->comm->rank]) { ops[o->comm->rank] = o; ++have; }
    if (have < K->nranks) continue;
    bool same = true;
    for (Op* o : ops) { take_out(o); same = same && o->count == ops[0]->count && o->type == ops[0]->type; }
    if (!same) {
      for (Op* o : ops) finish(o, ncclInvalidArgument, "ncclAllGather: the ranks differ in count or type");
    } else {
      const hipError_t e = run_gather(ops, ops[0]->count * type_size(ops[0]->type));
      for (Op* o : ops) finish(o, e == hipSuccess ? ncclSuccess : ncclUnhandledCudaError, e == hipSuccess ? nullptr : hipGetErrorString(e));
    }
    return true;
  }
  return false;
}

// Post ops (which stay where they are until this returns), execute what is complete, wait for the rest.
ncclResult_t post(std::vector<Op>& ops) {
  if (ops.empty()) return ncclSuccess;
  std::unique_lock<std::mutex> lk(g_mu);
  for (Op& o : ops) g_table.push_back(&o);
  {
    DeviceGuard keep;
    reap();
    while (match_one_pair() || match_one_gather()) {}
  }
  g_cv.notify_all();
  const auto all_done = [&] { for (const Op& o : ops) if (!o.done) return false; return true; };
  if (!g_cv.wait_for(lk, std::chrono::seconds(kRendezvousSeconds), all_done)) {
    for (Op& o : ops) if (!o.done) take_out(&o);
    return refuse(ncclInternalError, "internal error", "no matching call of the peer within the rendezvous bound");
  }
  for (const Op& o : ops)
    if (o.result != ncclSuccess) return refuse(o.result, o.result == ncclInvalidArgument ? "invalid argument" : "unhandled cuda error", o.why ? o.why : "?");
  return ncclSuccess;
}

ncclResult_t issue(const Op& o) {
  if (t_depth > 0) { t_queue.push_back(o); return ncclSuccess; }
  std::vector<Op> one(1, o);
  return post(one);
}

ncclComm* new_comm(Clique* K, int rank, int device) {
  ++K->live;
  ++g_live;
  return new ncclComm{K, rank, device};
}

void drop_comm(ncclComm* c) {
  if (--c->clique->live == 0) delete c->clique;
  --g_live;
  delete c;
}

}  // namespace

extern "C" int sl2_standin_live_comms(void) { return g_live.load(); }

ncclResult_t ncclGetUniqueId(ncclUniqueId* uniqueId) {
  if (!uniqueId) return invalid("ncclGetUniqueId: null");
  memset(uniqueId->internal, 0, sizeof(uniqueId->internal));
  const unsigned long long id = g_next_id.fetch_add(1);
  memcpy(uniqueId->internal, "standin", 8);
  memcpy(uniqueId->internal + 8, &id, sizeof(id));
  return ncclSuccess;
}

ncclResult_t ncclCommInitRank(ncclComm_t* comm, int nranks, ncclUniqueId commId, int rank) {
  if (!comm || nranks <= 0 || rank < 0 || rank >= nranks) return invalid("ncclCommInitRank: bad argument");
  int device = 0;
  if (hipGetDevice(&device) != hipSuccess) return refuse(ncclUnhandledCudaError, "unhandled cuda error", "hipGetDevice");
  const std::string key(commId.internal, sizeof(commId.internal));
  std::unique_lock<std::mutex> lk(g_mu);
  Clique*& slot = g_forming[key];
  if (!slot) { slot = new Clique(); slot->nranks = nranks; slot->joined.assign(nranks, false); }
  Clique* K = slot;
  if (K->nranks != nranks) return invalid("ncclCommInitRank: the ranks differ in nranks");
  if (K->joined[rank]) return invalid("ncclCommInitRank: this rank has already joined");   // (RCCL would hang)
  K->joined[rank] = true;
  ncclComm* c = new_comm(K, rank, device);
  if (K->live == nranks) {
    K->formed = true;
    g_forming.erase(key);
    g_cv.notify_all();
  } else if (!g_cv.wait_for(lk, std::chrono::seconds(kRendezvousSeconds), [&] { return K->formed; })) {
    K->joined[rank] = false;
    if (K->live == 1) g_forming.erase(key);
    drop_comm(c);
    return refuse(ncclInternalError, "internal error", "ncclCommInitRank: the peers did not arrive within the rendezvous bound");
  }
  *comm = c;
  return ncclSuccess;
}

ncclResult_t ncclCommInitAll(ncclComm_t* comm, int ndev, const int* devlist) {
  if (!comm || ndev <= 0) return invalid("ncclCommInitAll: bad argument");
  std::lock_guard<std::mutex> lk(g_mu);
  Clique* K = new Clique();
  K->nranks = ndev;
  K->formed = true;
  for (int i = 0; i < ndev; ++i) comm[i] = new_comm(K, i, devlist ? devlist[i] : i);   // the same device twice is fine here
  return ncclSuccess;
}

ncclResult_t ncclCommDestroy(ncclComm_t comm) {
  if (!comm) return ncclSuccess;
  std::lock_guard<std::mutex> lk(g_mu);
  for (size_t i = g_table.size(); i-- > 0;)
    if (g_table[i]->comm == comm) { finish(g_table[i], ncclInvalidArgument, "the communicator was destroyed"); g_table.erase(g_table.begin() + i); }
  g_cv.notify_all();
  drop_comm(comm);
  reap();
  return ncclSuccess;
}

const char* ncclGetErrorString(ncclResult_t result) {
  if (result != ncclSuccess && result == t_detail_code && !t_detail.empty()) return t_detail.c_str();
  switch (result) {
    case ncclSuccess: return "no error";
    case ncclUnhandledCudaError: return "unhandled cuda error";
    case ncclSystemError: return "unhandled system error";
    case ncclInternalError: return "internal error";
    case ncclInvalidArgument: return "invalid argument";
    case ncclInvalidUsage: return "invalid usage";
    default: return "unknown result code";
  }
}

ncclResult_t ncclGroupStart() {
  ++t_depth;
  return ncclSuccess;
}

ncclResult_t ncclGroupEnd() {
  if (t_depth <= 0) return invalid("ncclGroupEnd without ncclGroupStart");
  if (--t_depth > 0) return ncclSuccess;
  std::vector<Op> ops;
  ops.swap(t_queue);
  return post(ops);
}

ncclResult_t ncclSend(const void* sendbuff, size_t count, ncclDataType_t datatype, int peer, ncclComm_t comm, hipStream_t stream) {
  if (!comm || !type_size(datatype) || (count && !sendbuff)) return invalid("ncclSend: bad argument");
  if (peer < 0 || peer >= comm->clique->nranks) return invalid("ncclSend: peer out of range");
  return issue(Op{kSend, comm, sendbuff, nullptr, count, datatype, peer, stream});
}

ncclResult_t ncclRecv(void* recvbuff, size_t count, ncclDataType_t datatype, int peer, ncclComm_t comm, hipStream_t stream) {
  if (!comm || !type_size(datatype) || (count && !recvbuff)) return invalid("ncclRecv: bad argument");
  if (peer < 0 || peer >= comm->clique->nranks) return invalid("ncclRecv: peer out of range");
  return issue(Op{kRecv, comm, nullptr, recvbuff, count, datatype, peer, stream});
}

ncclResult_t ncclAllGather(const void* sendbuff, void* recvbuff, size_t sendcount, ncclDataType_t datatype, ncclComm_t comm,
                           hipStream_t stream) {
  if (!comm || !type_size(datatype) || (sendcount && (!sendbuff || !recvbuff))) return invalid("ncclAllGather: bad argument");
  return issue(Op{kGather, comm, sendbuff, recvbuff, sendcount, datatype, -1, stream});
}
