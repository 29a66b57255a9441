// elfrq_dev_*: the device side of ElfReaderQueues -- a mirror of the queues in device memory, one mt19937 per game thread beside
// it, and the launches of k_rq_draw / k_rq_scatter (rq_draw.cuh).  The host queues and elfrq_draw stay record_host.cpp's;
// rq_host.h is what the two share.  An object of its own (GNUmakefile): nothing here includes the board kernels.
#include <sstream>
#include <vector>

#include "rq_draw.cuh"
#include "rq_host.h"

#define HIPCHK(x)                         \
  do {                                    \
    hipError_t _e = (x);                  \
    if (_e != hipSuccess) return (int)_e; \
  } while (0)

namespace {
// the device of a handle for an entry's duration, then the caller's again (engine_host.h's DevGuard)
struct DevGuard {
  int prev = -1;
  explicit DevGuard(int dev) {
    int cur = -1;
    if (hipGetDevice(&cur) == hipSuccess && cur != dev && hipSetDevice(dev) == hipSuccess) prev = cur;
  }
  ~DevGuard() { if (prev >= 0) (void)hipSetDevice(prev); }
  DevGuard(const DevGuard&) = delete;
  DevGuard& operator=(const DevGuard&) = delete;
};
}  // namespace

struct ElfRqDevice {
  ElfReaderQueues* q = nullptr;
  int device = 0, T = 0;
  rq::Mirror m{};
  uint32_t* d_mt = nullptr;      // [T][624]
  uint32_t* d_pos = nullptr;     // [T]
  uint32_t* d_stuck = nullptr;   // sticky: a state ran into the retry bound
  int64_t next_act = 0;          // the handle's own turn counter
  bool min_size_satisfied = false;
  int eligible_nfa = 0;          // the num_future_actions an eligible record is known to exist for (0 = not known)
  // an update travels pinned host chunk -> device chunk -> k_rq_scatter; a pair is reused once its event (behind the kernel) is over
  struct Stage { int32_t* host = nullptr; int32_t* dev = nullptr; hipEvent_t done = nullptr; } stage[2];
  int turn = 0;
  size_t chunk_ints = 0;
};

namespace {

void rq_free(ElfRqDevice* d) {
  (void)hipFree(d->m.ring); (void)hipFree(d->m.head); (void)hipFree(d->m.size);
  (void)hipFree(d->d_mt); (void)hipFree(d->d_pos); (void)hipFree(d->d_stuck);
  for (auto& s : d->stage) {
    if (s.host) (void)hipHostFree(s.host);
    if (s.dev) (void)hipFree(s.dev);
    if (s.done) (void)hipEventDestroy(s.done);
  }
  delete d;
}

// Sends heads, sizes and the records at the noted ring positions (all records after an overflow of the list), CHUNK at a time.
int rq_update(ElfRqDevice* d, hipStream_t s) {
  ElfReaderQueues* q = d->q;
  const int nq = d->m.nq, qmax = d->m.qmax, at = rq::chunk_entries_at(nq);
  if (q->pending_all) {
    q->pending.clear();
    for (int i = 0; i < nq; ++i)
      for (size_t j = 0; j < q->qs[(size_t)i].size(); ++j) q->pending.push_back({i, (int32_t)((q->ring_head[(size_t)i] + (int64_t)j) % qmax)});
  }
  const size_t total = q->pending.size();
  for (size_t done = 0; done == 0 || done < total; done += rq::CHUNK) {
    ElfRqDevice::Stage& st = d->stage[d->turn];
    d->turn ^= 1;
    HIPCHK(hipEventSynchronize(st.done));
    const int n = (int)std::min<size_t>(rq::CHUNK, total - done);
    st.host[0] = n;
    for (int i = 0; i < nq; ++i) { st.host[1 + i] = q->ring_head[(size_t)i]; st.host[1 + nq + i] = (int32_t)q->qs[(size_t)i].size(); }
    for (int k = 0; k < n; ++k) {
      const ElfReaderQueues::Touched t = q->pending[done + (size_t)k];
      // the record that is at that ring position now: deque element (pos - head) mod qmax
      const ElfReaderQueues::Rec r = q->qs[(size_t)t.queue][(size_t)(((int64_t)t.pos - q->ring_head[(size_t)t.queue] + qmax) % qmax)];
      int32_t* e = st.host + at + 4 * k;
      e[0] = t.queue; e[1] = t.pos; e[2] = r.slot; e[3] = r.num_moves;
    }
    HIPCHK(hipMemcpyAsync(st.dev, st.host, sizeof(int32_t) * ((size_t)at + 4 * (size_t)n), hipMemcpyHostToDevice, s));
    const int items = std::max(n, nq);
    hipLaunchKernelGGL(rq::k_rq_scatter, dim3((items + 255) / 256), dim3(256), 0, s, d->m, (const int32_t*)st.dev);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(st.done, s));
  }
  q->pending.clear();
  q->pending_all = false;
  q->mirror_stale = false;
  return 0;
}

}  // namespace

extern "C" {

int elfrq_dev_create(ElfReaderQueues* q, int device, ElfRqDevice** out) {
  if (!q || !out || q->dev || device < 0 || q->qs.size() > (size_t)rq::MAX_QUEUES || q->queue_max_size > ((size_t)1 << 30)) return ELFGO_E_BADARG;
  DevGuard _dg(device);
  ElfRqDevice* d = new ElfRqDevice();
  d->q = q;
  d->device = device;
  d->T = (int)q->thread_rng.size();
  d->m.nq = (int)q->qs.size();
  d->m.qmax = (int)q->queue_max_size;
  d->m.qmin = (int)q->queue_min_size;
  d->next_act = q->next_act;
  d->min_size_satisfied = q->min_size_satisfied;
  const int nq = d->m.nq, qmax = d->m.qmax, T = d->T;
  // every generator as operator<< writes it: 624 state words, then the position
  std::vector<uint32_t> mt((size_t)T * rq::MT_N), pos((size_t)T);
  for (int t = 0; t < T; ++t) {
    std::stringstream ss;
    ss << q->thread_rng[(size_t)t];
    uint64_t v = 0;
    for (int i = 0; i < rq::MT_N; ++i) { ss >> v; mt[(size_t)t * rq::MT_N + i] = (uint32_t)v; }
    ss >> v;
    if (!ss || v > (uint64_t)rq::MT_N) { delete d; return ELFGO_E_BADARG; }
    pos[(size_t)t] = (uint32_t)v;
  }
  // the queues as they are: every ring starts at position 0
  std::vector<int2> ring((size_t)nq * qmax, make_int2(0, 0));
  std::vector<int32_t> head((size_t)nq, 0), size((size_t)nq);
  for (int i = 0; i < nq; ++i) {
    size[(size_t)i] = (int32_t)q->qs[(size_t)i].size();
    for (size_t j = 0; j < q->qs[(size_t)i].size(); ++j) ring[(size_t)i * qmax + j] = make_int2(q->qs[(size_t)i][j].slot, q->qs[(size_t)i][j].num_moves);
  }
  d->chunk_ints = (size_t)rq::chunk_entries_at(nq) + 4 * (size_t)rq::CHUNK;
  const uint32_t zero = 0;
  hipError_t he = hipMalloc((void**)&d->m.ring, ring.size() * sizeof(int2));
  if (he == hipSuccess) he = hipMalloc((void**)&d->m.head, sizeof(int32_t) * nq);
  if (he == hipSuccess) he = hipMalloc((void**)&d->m.size, sizeof(int32_t) * nq);
  if (he == hipSuccess) he = hipMalloc((void**)&d->d_mt, mt.size() * sizeof(uint32_t));
  if (he == hipSuccess) he = hipMalloc((void**)&d->d_pos, pos.size() * sizeof(uint32_t));
  if (he == hipSuccess) he = hipMalloc((void**)&d->d_stuck, sizeof(uint32_t));
  for (auto& s : d->stage) {
    if (he == hipSuccess) he = hipHostMalloc((void**)&s.host, d->chunk_ints * sizeof(int32_t), hipHostMallocDefault);
    if (he == hipSuccess) he = hipMalloc((void**)&s.dev, d->chunk_ints * sizeof(int32_t));
    if (he == hipSuccess) he = hipEventCreateWithFlags(&s.done, hipEventDisableTiming);
  }
  if (he == hipSuccess) he = hipMemcpy(d->m.ring, ring.data(), ring.size() * sizeof(int2), hipMemcpyHostToDevice);
  if (he == hipSuccess) he = hipMemcpy(d->m.head, head.data(), sizeof(int32_t) * nq, hipMemcpyHostToDevice);
  if (he == hipSuccess) he = hipMemcpy(d->m.size, size.data(), sizeof(int32_t) * nq, hipMemcpyHostToDevice);
  if (he == hipSuccess) he = hipMemcpy(d->d_mt, mt.data(), mt.size() * sizeof(uint32_t), hipMemcpyHostToDevice);
  if (he == hipSuccess) he = hipMemcpy(d->d_pos, pos.data(), pos.size() * sizeof(uint32_t), hipMemcpyHostToDevice);
  if (he == hipSuccess) he = hipMemcpy(d->d_stuck, &zero, sizeof(zero), hipMemcpyHostToDevice);
  if (he != hipSuccess) { rq_free(d); return (int)he; }
  q->ring_head.assign((size_t)nq, 0);
  q->pending.clear();
  q->pending_all = false;
  q->mirror_stale = false;
  q->dev = d;
  *out = d;
  return 0;
}

int elfrq_dev_destroy(ElfRqDevice* d) {
  if (!d) return ELFGO_E_BADARG;
  DevGuard _dg(d->device);
  (void)hipDeviceSynchronize();   // draws and updates still queued read what is freed here
  d->q->dev = nullptr;
  d->q->pending.clear();
  d->q->pending_all = false;
  rq_free(d);
  return 0;
}

int elfrq_dev_draw(ElfRqDevice* d, int num_acts, int num_future_actions, int32_t* dev_slot, int32_t* dev_move_to, int32_t* dev_d4, void* stream) {
  if (!d || num_acts < 0 || num_future_actions < 1 || !dev_slot || !dev_move_to || !dev_d4) return ELFGO_E_BADARG;
  ElfReaderQueues* q = d->q;
  // elfrq_draw's two refusals, on the host queues (which the mirror equals once it is up to date)
  if (!d->min_size_satisfied) {
    for (const auto& b : q->qs) if (b.size() < q->queue_min_size) return ELFGO_E_BADARG;
    d->min_size_satisfied = true;
  }
  if (q->mirror_stale || d->eligible_nfa != num_future_actions) {   // queues only change by inserts: asked once per change
    bool any = false;
    for (const auto& b : q->qs)
      if (b.size() >= q->queue_min_size)
        for (const auto& r : b) any = any || r.num_moves > num_future_actions - 1;
    d->eligible_nfa = any ? num_future_actions : 0;
    if (!any) return ELFGO_E_BADARG;
  }
  DevGuard _dg(d->device);
  hipStream_t s = (hipStream_t)stream;
  if (q->mirror_stale) {
    const int rc = rq_update(d, s);
    if (rc) return rc;
  }
  if (num_acts == 0) return 0;
  // even_ratio as getSamplerWithParity computes it: constant during a call
  const float kSafeMargin = 0.45;
  const int even = q->parity_sizes[0], odd = q->parity_sizes[1];
  float even_ratio = static_cast<float>(even) / (even + odd + 1e-6);
  even_ratio = std::max(even_ratio, kSafeMargin);
  even_ratio = std::min(even_ratio, 1.0f - kSafeMargin);
  const int first = (int)(d->next_act % d->T);
  hipLaunchKernelGGL(rq::k_rq_draw, dim3(d->T), dim3(64), sizeof(int32_t) * 2 * (size_t)d->m.nq, s, d->m, d->d_mt, d->d_pos, d->T, first,
                     num_acts, num_future_actions, even_ratio, dev_slot, dev_move_to, dev_d4, d->d_stuck);
  HIPCHK(hipGetLastError());
  d->next_act += num_acts;
  return 0;
}

int elfrq_dev_status(ElfRqDevice* d, void* stream) {
  if (!d) return ELFGO_E_BADARG;
  DevGuard _dg(d->device);
  uint32_t stuck = 0;
  HIPCHK(hipStreamSynchronize((hipStream_t)stream));
  HIPCHK(hipMemcpy(&stuck, d->d_stuck, sizeof(stuck), hipMemcpyDeviceToHost));
  return stuck ? ELFGO_E_NODATA : 0;
}

}  // extern "C"
