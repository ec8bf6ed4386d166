// gpx_shard.inc — row-block-cyclic shard of the Gram matrix over P GPUs, one process per
// GPU (SURVEY.md §8e, row "K5").  Included by gpx_api.hip (same translation unit).
//
// Distribution: row blocks of height nb, dealt over the ranks by gpx_internal.h's Deal (snake by default: rounds of
// 2 P blocks go 0 .. P-1, P-1 .. 0, which balances the row work; GPX_SHARD_DEAL=cyclic: block g on rank g % P); every rank stores its rows full width ([nloc][ld]).  X (N x d) is
// replicated (1.5 MiB at N = 65536), so kernel build, K*, mean and variance partials need
// no exchange; the factorisation has ONE exchange step per panel:
//   1. owner(p) factors the diagonal block (two-level POTF2 as on one GPU)
//   2. broadcast  [L_pp | Winv_pp]                      (nb*nb + nb*64 doubles)
//   3. every rank solves its own rows of panel p        (trsm_rlt, local)
//   4. all-gather of the panel columns                  ((n - o - nb) * nb doubles in total)
//   5. every rank updates its own trailing rows         (gemm_nt, block-cyclic tile mask)
// Triangular solves exchange one (rows x nb) block per panel: forward = broadcast of
// the solved block; backward = reduce of the partial products to the owner.
//
// Transport: RCCL (`librccl.so.1`, resolved at run time so that a single-GPU process
// never loads it) on the handle's stream, or caller-supplied host collectives
// (gpx_comm_init_host) with device<->host staging — the latter exists so that the
// schedule can be exercised by several processes sharing ONE GPU (tests), where RCCL
// refuses duplicate devices.

#include <dlfcn.h>

#include <condition_variable>
#include <mutex>
#include <thread>

namespace {

enum { COMM_SUM = 0, COMM_MIN = 1 };

struct Comm {
  int rank = 0, world = 1;
  virtual ~Comm() {}
  // all buffers are device memory; calls are ordered on stream `st` (nullptr = h->st).  Broadcast and all-gather move
  // bytes; the reductions are typed (f32 != 0: float, else double) — the shard runs in the handle's element type.
  virtual int bcast_bytes(gpx_handle* h, void* buf, size_t bytes, int root, hipStream_t st) = 0;
  virtual int allgather_bytes(gpx_handle* h, const void* send, void* recv, size_t bytes_per_rank, hipStream_t st) = 0;
  virtual int reduce_any(gpx_handle* h, const void* send, void* recv, size_t count, int root, int op, int f32) = 0;
  virtual int allreduce_any(gpx_handle* h, void* buf, size_t count, int op, int f32) = 0;
  template <typename T>
  int bcast(gpx_handle* h, T* buf, size_t count, int root, hipStream_t st = nullptr) {
    return bcast_bytes(h, buf, count * sizeof(T), root, st);
  }
  template <typename T>
  int allgather(gpx_handle* h, const T* send, T* recv, size_t count_per_rank, hipStream_t st = nullptr) {
    return allgather_bytes(h, send, recv, count_per_rank * sizeof(T), st);
  }
  template <typename T>
  int reduce(gpx_handle* h, const T* send, T* recv, size_t count, int root, int op) {
    return reduce_any(h, send, recv, count, root, op, sizeof(T) == 4);
  }
  template <typename T>
  int allreduce(gpx_handle* h, T* buf, size_t count, int op) {
    return allreduce_any(h, buf, count, op, sizeof(T) == 4);
  }
};

// ---- RCCL ---------------------------------------------------------------------------------
struct Id128 {  // ncclUniqueId (NCCL_UNIQUE_ID_BYTES = 128), passed by value
  char b[128];
};
struct RcclApi {
  void* lib = nullptr;
  int (*GetUniqueId)(void*) = nullptr;
  int (*CommInitRank)(void**, int, Id128, int) = nullptr;
  int (*CommInitAll)(void**, int, const int*) = nullptr;
  int (*GroupStart)() = nullptr;
  int (*GroupEnd)() = nullptr;
  int (*CommDestroy)(void*) = nullptr;
  int (*Broadcast)(const void*, void*, size_t, int, int, void*, hipStream_t) = nullptr;
  int (*AllGather)(const void*, void*, size_t, int, void*, hipStream_t) = nullptr;
  int (*Reduce)(const void*, void*, size_t, int, int, int, void*, hipStream_t) = nullptr;
  int (*AllReduce)(const void*, void*, size_t, int, int, void*, hipStream_t) = nullptr;
  const char* (*GetErrorString)(int) = nullptr;
};
constexpr int NCCL_I8 = 0, NCCL_F32 = 7, NCCL_F64 = 8, NCCL_SUM = 0, NCCL_MIN = 3;

RcclApi* rccl_api(std::string* err) {
  static RcclApi api;
  static bool tried = false;
  if (api.lib) return &api;
  if (tried) {
    if (err) *err = "librccl could not be loaded";
    return nullptr;
  }
  tried = true;
  // ONE RCCL per process, and torch's first: if a copy is already mapped (PyTorch-ROCm wheels bundle
  // their own and map it with `import torch`), use that one.  A process that dlopen()s an RCCL here
  // BEFORE importing torch aborts at exit (static destructors: "double free or corruption", round 3,
  // tools/rccl_exit_probe.py), so the Python host imports torch and points GPX_RCCL_PATH at its copy
  // before the first RCCL use (_abi.prefer_torch_rccl).
  EnvKnobs env;
  env_read(env, EnvAt::process);
  const char* names[] = {env.rccl_path, "librccl.so.1", "librccl.so"};
  for (const char* n : names) {
    if (!n || !*n) continue;
    api.lib = dlopen(n, RTLD_NOW | RTLD_GLOBAL | RTLD_NOLOAD);
    if (api.lib) break;
  }
  for (const char* n : names) {
    if (api.lib) break;
    if (!n || !*n) continue;
    api.lib = dlopen(n, RTLD_NOW | RTLD_GLOBAL);
  }
  if (!api.lib) {
    if (err) *err = std::string("dlopen(librccl) failed: ") + dlerror();
    return nullptr;
  }
#define RSYM(field, name)                                                      \
  api.field = reinterpret_cast<decltype(api.field)>(dlsym(api.lib, name));    \
  if (!api.field) {                                                            \
    if (err) *err = std::string("librccl lacks ") + name;                      \
    api.lib = nullptr;                                                         \
    return nullptr;                                                            \
  }
  RSYM(GetUniqueId, "ncclGetUniqueId")
  RSYM(CommInitRank, "ncclCommInitRank")
  RSYM(CommInitAll, "ncclCommInitAll")
  RSYM(GroupStart, "ncclGroupStart")
  RSYM(GroupEnd, "ncclGroupEnd")
  RSYM(CommDestroy, "ncclCommDestroy")
  RSYM(Broadcast, "ncclBroadcast")
  RSYM(AllGather, "ncclAllGather")
  RSYM(Reduce, "ncclReduce")
  RSYM(AllReduce, "ncclAllReduce")
  RSYM(GetErrorString, "ncclGetErrorString")
#undef RSYM
  return &api;
}

struct RcclComm : Comm {
  RcclApi* api = nullptr;
  void* comm = nullptr;
  ~RcclComm() override {
    if (api && comm) api->CommDestroy(comm);
  }
  int chk(gpx_handle* h, int rc, const char* what) {
    if (rc == 0) return GPX_OK;
    h->err = std::string(what) + " failed: " + api->GetErrorString(rc);
    return GPX_E_COMM;
  }
  int bcast_bytes(gpx_handle* h, void* buf, size_t bytes, int root, hipStream_t st) override {
    return chk(h, api->Broadcast(buf, buf, bytes, NCCL_I8, root, comm, st ? st : h->st), "ncclBroadcast");
  }
  int allgather_bytes(gpx_handle* h, const void* send, void* recv, size_t bytes, hipStream_t st) override {
    return chk(h, api->AllGather(send, recv, bytes, NCCL_I8, comm, st ? st : h->st), "ncclAllGather");
  }
  int reduce_any(gpx_handle* h, const void* send, void* recv, size_t count, int root, int op, int f32) override {
    return chk(h, api->Reduce(send, recv, count, f32 ? NCCL_F32 : NCCL_F64, op == COMM_MIN ? NCCL_MIN : NCCL_SUM, root,
                              comm, h->st), "ncclReduce");
  }
  int allreduce_any(gpx_handle* h, void* buf, size_t count, int op, int f32) override {
    return chk(h, api->AllReduce(buf, buf, count, f32 ? NCCL_F32 : NCCL_F64, op == COMM_MIN ? NCCL_MIN : NCCL_SUM,
                                 comm, h->st), "ncclAllReduce");
  }
};

// ---- host-callback transport -----------------------------------------------------------------
struct HostComm : Comm {
  gpx_host_comm vt{};
  void* stage = nullptr;  // pinned host staging
  size_t cap = 0;
  ~HostComm() override {
    if (stage) (void)hipHostFree(stage);
  }
  int need(gpx_handle* h, size_t bytes) {
    if (cap >= bytes) return GPX_OK;
    if (stage) (void)hipHostFree(stage);
    stage = nullptr;
    cap = 0;
    HIPCHK(h, hipHostMalloc(&stage, bytes, hipHostMallocDefault));
    cap = bytes;
    return GPX_OK;
  }
  int cb(gpx_handle* h, int rc, const char* what) {
    if (rc == 0) return GPX_OK;
    h->err = std::string("host collective ") + what + " returned " + std::to_string(rc);
    return GPX_E_COMM;
  }
  int bcast_bytes(gpx_handle* h, void* buf, size_t bytes, int root, hipStream_t st_) override {
    hipStream_t st = st_ ? st_ : h->st;
    int rc;
    if ((rc = need(h, bytes))) return rc;
    if (rank == root) {
      HIPCHK(h, hipMemcpyAsync(stage, buf, bytes, hipMemcpyDeviceToHost, st));
    }
    HIPCHK(h, hipStreamSynchronize(st));
    if ((rc = cb(h, vt.bcast(vt.ctx, stage, (int64_t)bytes, root), "bcast"))) return rc;
    if (rank != root) HIPCHK(h, hipMemcpyAsync(buf, stage, bytes, hipMemcpyHostToDevice, st));
    HIPCHK(h, hipStreamSynchronize(st));
    return GPX_OK;
  }
  int allgather_bytes(gpx_handle* h, const void* send, void* recv, size_t b, hipStream_t st_) override {
    hipStream_t st = st_ ? st_ : h->st;
    int rc;
    if ((rc = need(h, b * (world + 1)))) return rc;
    char* s = (char*)stage;
    HIPCHK(h, hipMemcpyAsync(s, send, b, hipMemcpyDeviceToHost, st));
    HIPCHK(h, hipStreamSynchronize(st));
    if ((rc = cb(h, vt.allgather(vt.ctx, s, s + b, (int64_t)b), "allgather"))) return rc;
    HIPCHK(h, hipMemcpyAsync(recv, s + b, b * world, hipMemcpyHostToDevice, st));
    HIPCHK(h, hipStreamSynchronize(st));
    return GPX_OK;
  }
  // the caller's callbacks reduce doubles (include/gpx.h): fp32 shards widen on the host and narrow the result
  // (a sum of P floats formed in double and rounded once: at least as accurate as the float sum of the other transports)
  int reduce_any(gpx_handle* h, const void* send, void* recv, size_t count, int root, int op, int f32) override {
    int rc;
    const size_t b = count * 8, bin = count * (f32 ? 4 : 8);
    if ((rc = need(h, 3 * b))) return rc;
    char* s = (char*)stage;
    HIPCHK(h, hipMemcpyAsync(s + 2 * b, send, bin, hipMemcpyDeviceToHost, h->st));
    HIPCHK(h, hipStreamSynchronize(h->st));
    double* in = (double*)s;
    if (f32)
      for (size_t i = 0; i < count; ++i) in[i] = (double)((const float*)(s + 2 * b))[i];
    else
      memcpy(in, s + 2 * b, b);
    if ((rc = cb(h, vt.reduce(vt.ctx, in, (double*)(s + b), (int64_t)count, root, op), "reduce"))) return rc;
    if (rank == root) {
      if (f32)
        for (size_t i = 0; i < count; ++i) ((float*)(s + 2 * b))[i] = (float)((const double*)(s + b))[i];
      HIPCHK(h, hipMemcpyAsync(recv, f32 ? s + 2 * b : s + b, bin, hipMemcpyHostToDevice, h->st));
    }
    HIPCHK(h, hipStreamSynchronize(h->st));
    return GPX_OK;
  }
  int allreduce_any(gpx_handle* h, void* buf, size_t count, int op, int f32) override {
    int rc;
    const size_t b = count * 8, bin = count * (f32 ? 4 : 8);
    if ((rc = need(h, 2 * b))) return rc;
    char* s = (char*)stage;
    HIPCHK(h, hipMemcpyAsync(s + b, buf, bin, hipMemcpyDeviceToHost, h->st));
    HIPCHK(h, hipStreamSynchronize(h->st));
    double* v = (double*)s;
    if (f32)
      for (size_t i = 0; i < count; ++i) v[i] = (double)((const float*)(s + b))[i];
    else
      memcpy(v, s + b, b);
    if ((rc = cb(h, vt.allreduce(vt.ctx, v, (int64_t)count, op), "allreduce"))) return rc;
    if (f32)
      for (size_t i = 0; i < count; ++i) ((float*)(s + b))[i] = (float)v[i];
    HIPCHK(h, hipMemcpyAsync(buf, f32 ? (void*)(s + b) : (void*)v, bin, hipMemcpyHostToDevice, h->st));
    HIPCHK(h, hipStreamSynchronize(h->st));
    return GPX_OK;
  }
};


// ---- in-process transport of a device group ----------------------------------------------------
// The ranks of a single-process group (gpx_config.ndev) are threads of one process, so a
// collective needs no library: a rank PULLS what it needs straight out of its peers' device
// buffers with a (peer) copy on its own stream, ordered by hipEvents between the ranks' streams.
// On the xGMI full mesh that is the all-gather SURVEY.md §5 asks for — every GPU reads its 7
// peers' pieces over 7 links at once instead of walking a ring.  The host threads meet at a
// barrier twice per collective (publish pointers + "ready" events; publish "done" events), but
// never wait for the GPU: everything stays asynchronous on the stream the schedule chose, so
// the look-ahead stream's exchanges really run beside the trailing update of the main stream.
// Several ranks may list the SAME device (tests: 8 ranks on one GPU).
struct LocalHub {
  struct Pub {
    const void* ptr;
    hipEvent_t ev;
  };
  int P = 0;
  std::vector<int> dev;          // HIP ordinal of every rank
  std::vector<Pub> pub;          // written before barrier A, read between A and B
  std::vector<hipEvent_t> done;  // written between A and B, read after B
  std::mutex mu;
  std::condition_variable cv;
  int arrived = 0;
  uint64_t gen = 0;
  bool aborted = false;
  void init(int P_) {
    P = P_;
    dev.assign(P, 0);
    pub.assign(P, Pub{nullptr, nullptr});
    done.assign(P, nullptr);
  }
  void reset() {  // start of a group call: every member thread is outside
    std::lock_guard<std::mutex> lk(mu);
    arrived = 0;
    aborted = false;
  }
  void abort() {  // a rank failed: wake everybody, every later barrier fails at once
    std::lock_guard<std::mutex> lk(mu);
    aborted = true;
    cv.notify_all();
  }
  bool barrier() {  // false: the group was aborted (a peer failed)
    std::unique_lock<std::mutex> lk(mu);
    if (aborted) return false;
    const uint64_t g = gen;
    if (++arrived == P) {
      arrived = 0;
      ++gen;
      cv.notify_all();
      return true;
    }
    cv.wait(lk, [&] { return gen != g || aborted; });
    return gen != g;
  }
};

struct LocalComm : Comm {
  LocalHub* hub = nullptr;
  DevBuf scratch;  // world x count staging of the reductions (element type of the call)
  int lost(gpx_handle* h) {
    if (h->err.empty()) h->err = "device group aborted: another rank failed";
    return GPX_E_COMM;
  }
#define LCHK(call)                                                                            \
  do {                                                                                        \
    hipError_t e_ = (call);                                                                   \
    if (e_ != hipSuccess) {                                                                   \
      h->err = std::string(#call " failed: ") + hipGetErrorString(e_) + " (local transport)"; \
      hub->abort();                                                                           \
      return GPX_E_HIP;                                                                       \
    }                                                                                         \
  } while (0)
  int record(gpx_handle* h, hipStream_t st, hipEvent_t* out) {
    hipEvent_t e = next_event(h);
    if (!e) {
      h->err = "hipEventCreate failed (local transport)";
      hub->abort();
      return GPX_E_HIP;
    }
    debug_delay(st);  // (test hook) the published data becomes "ready" later
    LCHK(hipEventRecord(e, st));
    *out = e;
    return GPX_OK;
  }
  int pull(gpx_handle* h, void* dst, int q, size_t bytes, hipStream_t st) {  // after barrier A
    debug_delay(st);    // (test hook) this rank arrives later
    LCHK(hipStreamWaitEvent(st, hub->pub[q].ev, 0));
    // (GPX_LOCAL_FORCE_PEER=1, test hook: the peer-copy call also between ranks that share a device — the only way a
    //  one-GPU box executes that line at all; with equal ordinals it is an ordinary copy)
    if (hub->dev[q] == hub->dev[rank] && !h->env.local_force_peer)
      LCHK(hipMemcpyAsync(dst, hub->pub[q].ptr, bytes, hipMemcpyDeviceToDevice, st));
    else
      LCHK(hipMemcpyPeerAsync(dst, hub->dev[rank], hub->pub[q].ptr, hub->dev[q], bytes, st));
    return GPX_OK;
  }
  int bcast_bytes(gpx_handle* h, void* buf, size_t bytes, int root, hipStream_t st_) override {
    hipStream_t st = st_ ? st_ : h->st;
    int rc;
    if (rank == root) {
      hipEvent_t e;
      if ((rc = record(h, st, &e))) return rc;
      hub->pub[rank] = {buf, e};
    }
    if (!hub->barrier()) return lost(h);
    if (rank != root) {
      if ((rc = pull(h, buf, root, bytes, st))) return rc;
      if ((rc = record(h, st, &hub->done[rank]))) return rc;
    }
    if (!hub->barrier()) return lost(h);
    if (rank == root)  // the root may overwrite buf only after every rank has read it
      for (int q = 0; q < world; ++q)
        if (q != root) LCHK(hipStreamWaitEvent(st, hub->done[q], 0));
    return GPX_OK;
  }
  int allgather_bytes(gpx_handle* h, const void* send, void* recv, size_t bytes, hipStream_t st_) override {
    hipStream_t st = st_ ? st_ : h->st;
    int rc;
    hipEvent_t e;
    if ((rc = record(h, st, &e))) return rc;
    hub->pub[rank] = {send, e};
    if (!hub->barrier()) return lost(h);
    for (int i = 0; i < world; ++i) {
      const int q = (rank + i) % world;  // own piece first, then the peers, staggered
      if ((rc = pull(h, (char*)recv + (size_t)q * bytes, q, bytes, st))) return rc;
    }
    if ((rc = record(h, st, &hub->done[rank]))) return rc;
    if (!hub->barrier()) return lost(h);
    for (int q = 0; q < world; ++q)
      if (q != rank) LCHK(hipStreamWaitEvent(st, hub->done[q], 0));
    return GPX_OK;
  }
  // every rank in `who` (root, or -1 = all) ends up with op over the ranks, summed in rank
  // order: all ranks get bit-identical results
  int reduce_impl(gpx_handle* h, const void* send, void* recv, size_t count, int root, int op, int f32) {
    hipStream_t st = h->st;
    const size_t es = f32 ? 4 : 8;
    int rc;
    hipEvent_t e;
    if ((rc = record(h, st, &e))) return rc;
    hub->pub[rank] = {send, e};
    const bool mine = root < 0 || rank == root;
    if (mine && (rc = ensure(h, scratch, (size_t)world * count * es))) {
      hub->abort();
      return rc;
    }
    if (!hub->barrier()) return lost(h);
    if (mine)
      for (int q = 0; q < world; ++q)
        if ((rc = pull(h, (char*)scratch.p + (size_t)q * count * es, q, count * es, st))) return rc;
    if ((rc = record(h, st, &hub->done[rank]))) return rc;
    if (!hub->barrier()) return lost(h);
    for (int q = 0; q < world; ++q)  // send buffers (== recv for an all-reduce) are free again
      if (q != rank && (root < 0 || q == root)) LCHK(hipStreamWaitEvent(st, hub->done[q], 0));
    if (mine) {
      if (f32)
        launch_reduce_ranks<float>((const float*)scratch.p, (float*)recv, world, (int64_t)count, op, st);
      else
        launch_reduce_ranks<double>((const double*)scratch.p, (double*)recv, world, (int64_t)count, op, st);
    }
    return GPX_OK;
  }
  int reduce_any(gpx_handle* h, const void* send, void* recv, size_t count, int root, int op, int f32) override {
    return reduce_impl(h, send, recv, count, root, op, f32);
  }
  int allreduce_any(gpx_handle* h, void* buf, size_t count, int op, int f32) override {
    return reduce_impl(h, buf, buf, count, -1, op, f32);
  }
#undef LCHK
};

// ---- bookkeeping of the dealing (gpx_internal.h: Deal — cyclic or snake) --------------------------------------------
struct Shard {
  int P, r, nb;
  int64_t nblk;
  int snake = 1;
  Deal deal() const { return Deal{P, snake}; }
  int owner(int64_t g) const { return deal().owner(g); }
  int64_t local(int64_t g) const { return deal().local(g); }                // index of block g among its owner's blocks
  int64_t global(int rr, int64_t lb) const { return deal().global(rr, lb); }  // block number lb of rank rr
  // number of blocks owned by rr with global index <= p
  int64_t lb0(int64_t p, int rr) const { return deal().upto(p, rr); }
  int64_t nlb(int rr) const { return lb0(nblk - 1, rr); }  // blocks owned by rr
  int64_t maxcnt(int64_t p) const {  // max over ranks of trailing local rows after panel p
    int64_t m = 0;
    for (int rr = 0; rr < P; ++rr) m = std::max(m, (nlb(rr) - lb0(p, rr)) * nb);
    return m;
  }
  // the staircase of this rank's launch: local rows from block number lbf on, columns from block gc0 on; piece > 0: the B
  // operand is the all-gathered panel p in rank-major pieces of `piece` rows (bc_brow)
  BcMask mask(int tpb, int64_t lbf, int64_t gc0, int64_t p = 0, int64_t piece = 0) const {
    BcMask bc{P, tpb};
    bc.r = r;
    bc.lbf = (int)lbf;
    bc.gc0 = (int)gc0;
    bc.snake = snake;
    bc.p = (int)p;
    bc.piece = piece;
    return bc;
  }
};
#define COMMCHK(expr)                 \
  do {                                \
    int rc_ = (expr);                 \
    if (rc_ != GPX_OK) return rc_;    \
  } while (0)

template <typename T>
int shard_fwd_sweep(gpx_handle* h, const Shard& sh, T* VT, int64_t ldv, int64_t mp, int64_t p0, T* const SvB[2]);

// RT (64 rows x own columns, ldy: local column block lb = global block lb P + r) <- (L L^T)^-1 RT with the factor held
// DISTRIBUTED (h->K: own row blocks), then the result replicated in the global layout `full` (64 x ld) on every rank.
// Forward: the distributed sweep of the variance path on the 64 rows (one-block look-ahead); backward: per block the
// partial products are reduced to the owner, who solves its block.  Used by shard_fit (alpha) and by the mixed mode's
// refinement (delta = (L L^T)^-1 r per iteration).  Collective: every rank calls it.
template <typename T>
int shard_solve_dist(gpx_handle* h, const Shard& sh, T* RTloc, T* full, DevBuf* zfull = nullptr) {
  Comm* cm = h->comm;
  const int nb = sh.nb;
  const int64_t ld = h->ld, ldy = h->ldy;
  const int64_t nlb = sh.nlb(sh.r);
  const T* A = (const T*)h->K.p;
  const T* Winv = (const T*)h->Winv.p;
  T* Sbuf = (T*)h->Sbuf.p;
  T* Cneg = (T*)h->Cneg.p;
  gpx_timings& tm = h->tm;
  hipStream_t st = h->st;
  {
    T* SvF[2] = {Sbuf, Sbuf + (int64_t)RHS_ROWS * nb};
    COMMCHK(shard_fwd_sweep(h, sh, RTloc, ldy, RHS_ROWS, 0, SvF));
  }
  if (zfull) {  // the forward sweep's result z = L^-1 r, replicated in the global layout (gpx_fit_predict on a distributed shard)
    int rcz;
    if ((rcz = ensure(h, *zfull, (size_t)RHS_ROWS * ld * sizeof(T)))) return rcz;
    T* Z = (T*)zfull->p;
    HIPCHK(h, hipMemsetAsync(Z, 0, (size_t)RHS_ROWS * ld * sizeof(T), st));
    launch_scatter_local(RTloc, ldy, Z, ld, nb, (int)nlb, sh.deal(), sh.r, RHS_ROWS, st);
    PhaseScope pc(h, &tm.comm);
    COMMCHK(cm->allreduce(h, Z, (size_t)RHS_ROWS * ld, COMM_SUM));
  }
  HIPCHK(h, hipMemsetAsync(Cneg, 0, (size_t)RHS_ROWS * ld * sizeof(T), st));
  T* Sred = Sbuf + (int64_t)RHS_ROWS * nb;
  for (int64_t p = sh.nblk - 1; p >= 0; --p) {  // backward
    const int64_t o = p * nb, lo = sh.local(p) * nb;
    const int root = sh.owner(p);
    if (p + 1 < sh.nblk) {
      HIPCHK(h, hipMemcpy2DAsync(Sbuf, (size_t)nb * sizeof(T), Cneg + o, (size_t)ld * sizeof(T), (size_t)nb * sizeof(T),
                                 RHS_ROWS, hipMemcpyDeviceToDevice, st));
      PhaseScope pc(h, &tm.comm);
      COMMCHK(cm->reduce(h, Sbuf, Sred, (size_t)RHS_ROWS * nb, root, COMM_SUM));
    }
    if (sh.r == root) {
      if (p + 1 < sh.nblk) launch_add_block(RTloc + lo, ldy, Sred, nb, RHS_ROWS, nb, 1.0, st);
      launch_trsm_rln<T>(RTloc + lo, ldy, RHS_ROWS, A + lo * ld + o, ld, Winv + (o / KB) * (KB * KB), nb, st);
      if (o > 0) launch_gemm_nn(Cneg, ld, RTloc + lo, ldy, A + lo * ld, ld, RHS_ROWS, o, nb, st);
    }
  }
  HIPCHK(h, hipMemsetAsync(full, 0, (size_t)RHS_ROWS * ld * sizeof(T), st));
  launch_scatter_local(RTloc, ldy, full, ld, nb, (int)nlb, sh.deal(), sh.r, RHS_ROWS, st);
  {
    PhaseScope pc(h, &tm.comm);
    COMMCHK(cm->allreduce(h, full, (size_t)RHS_ROWS * ld, COMM_SUM));
  }
  return GPX_OK;
}

template <typename T>
int shard_fit(gpx_handle* h, const void* X, const void* y, int64_t N, int32_t d, int32_t k,
              const double* lengthscale, int32_t n_ls, double sf2, double sn2, double jitter,
              int32_t mem_kind, int64_t* info, bool retried = false, const void* Xq = nullptr, int64_t Mquery = 0) {
  // Xq != null (gpx_fit_predict on a shard, round 4): this rank's slice of the Mquery query points rides through the
  // factorisation as BORDERED rows of its local row set — K(Xq_r, X) in Mq more local rows behind the own blocks.  They
  // are "blocks" beyond the matrix: the panel solve of the own rows takes them along (contiguous rows), the staircase
  // map of the trailing update gives them every column, the all-gather leaves them out (they are nobody's B operand) —
  // and they leave the factorisation as V^T = (L^-1 K*^T)^T of the slice: the variance solve of predict costs no pass
  // and no per-block latency chain of its own.  Split schedule only (the caller checks).
  Comm* cm = h->comm;
  if (!cm) return fail(h, GPX_E_ARG, "gpx_fit: sharded handle without a communicator (call gpx_comm_init)");
  {  // device flags or hipEvents inside the owner's diagonal chain: rank-local (own streams only), probed once per handle
    const int prc = flag_handover_probe(h);
    if (prc != GPX_OK) return prc;
  }
  // Block height: wide blocks run the update kernel faster (k = nb: 68 TF at 1024, 63 at 512)
  // but cost balance — a row block's share of an update grows with its index and the last panels
  // idle P-1 ranks.  Cyclic dealing (rounds 1-3): at least 16 blocks per rank (the last rank is 8.4 % above the mean at
  // 16 blocks per rank, 17 % at 8); snake dealing (round 4): 0.65 % / 2.6 % in the same cases, so 8 blocks per rank
  // are enough — 1024 up to N / (8 P), down to 256 (tools/scaling_model.py: P = 8, N = 65536: fit 235 -> 223 -> 212 ms
  // for cyclic 512 / snake 512 / snake 1024).
  const EnvKnobs& env = h->env;  // the call's snapshot (gpx_env.h): nothing below reads the environment
  const int snake = env.shard_snake;  // the dealing: per fit (tests switch it), kept in the handle for everything that follows the fit
  int nb = 1024;
  while (nb > 256 && (int64_t)nb * (snake ? 8 : 16) * cm->world > N) nb >>= 1;
  if (env.nb_shard) nb = env.nb_shard;
  h->nb_shard = nb;
  Shard sh{cm->world, cm->rank, nb, 0};
  sh.snake = h->shard_snake = snake;
  const int64_t Npad = round_up(N, nb);
  sh.nblk = Npad / nb;
  const int64_t ld = Npad + ld_skew<T>(), ldp = nb + ld_skew<T>();
  const int64_t nlb = sh.nlb(sh.r), nloc = nlb * nb;
  const int64_t ldy = nloc + ld_skew<T>();
  const int64_t Mc = Xq ? round_up((Mquery + sh.P - 1) / sh.P, TILE) : 0;  // query points per rank (as shard_predict_repl)
  const int64_t mq0 = std::min<int64_t>(Mquery, (int64_t)sh.r * Mc), mq1 = std::min<int64_t>(Mquery, (int64_t)(sh.r + 1) * Mc);
  const int64_t Mr = Xq ? mq1 - mq0 : 0, Mq = round_up(Mr, TILE);  // this rank's slice, padded: the bordered rows
  h->fq_rows = Mq;
  const bool ride = Xq != nullptr;  // some rank carries query rows
  h->N = N; h->Npad = Npad; h->ld = ld; h->ldp = ldp; h->d = d; h->k = k; h->n_ls = n_ls;
  h->sf2 = sf2; h->sn2 = sn2; h->jitter = jitter;
  h->nloc = nloc; h->ldy = ldy;
  h->alphaT = nullptr;  // set below, once YT is allocated
  gpx_timings& tm = h->tm;
  tm.h2d = tm.kbuild = tm.chol = tm.solve = tm.logdet = tm.fit_total = 0;
  tm.chol_diag = tm.chol_trsm = tm.chol_strip = tm.chol_syrk = tm.syrk_flops = tm.comm = 0;
  tm.syrk_launches = 0;
  tm.kbuild_bytes = (double)sizeof(T) * ((double)N * (double)(N + 1) / 2.0 / sh.P + (double)N * d);
  const bool profile = (h->cfg.flags & GPX_FLAG_PROFILE) != 0;

  const int64_t maxcnt0 = sh.maxcnt(-1);  // the largest local row count
  int rc;
  if ((rc = ensure(h, h->X, (size_t)N * d * sizeof(T)))) return rc;
  if ((rc = ensure(h, h->Y, (size_t)N * k * sizeof(T)))) return rc;
  if ((rc = ensure(h, h->Xs, (size_t)Npad * d * sizeof(T)))) return rc;
  if ((rc = ensure(h, h->ls, MAX_D * 8))) return rc;
  if ((rc = ensure(h, h->K, (size_t)std::max<int64_t>(nloc + Mq, nb) * ld * sizeof(T)))) return rc;
  if (Mq > 0 && (rc = ensure_queries<T>(h, Mr))) return rc;
  if ((rc = ensure(h, h->Winv, (size_t)(Npad / KB) * KB * KB * sizeof(T)))) return rc;
  // two of each panel buffer: the look-ahead stream fills one set while the main stream
  // still reads the other
  const size_t plocE = (size_t)(maxcnt0 + Mq) * ldp, gE = (size_t)sh.P * maxcnt0 * ldp,
               dE = (size_t)2 * nb * nb + (size_t)nb * KB;  // [L_pp | 64-block inverses | W_p = L_pp^-1]
  if ((rc = ensure(h, h->P, 2 * plocE * sizeof(T)))) return rc;
  if ((rc = ensure(h, h->G, 2 * gE * sizeof(T)))) return rc;
  if ((rc = ensure(h, h->Dbuf, 2 * dE * sizeof(T)))) return rc;
  if ((rc = ensure(h, h->Sbuf, (size_t)RHS_ROWS * nb * 8 * 2))) return rc;
  if ((rc = ensure(h, h->Ublk, (size_t)nb * ldp * sizeof(T)))) return rc;  // scratch of the block inverse in flight
  if ((rc = ensure(h, h->YTloc, (size_t)RHS_ROWS * ldy * sizeof(T)))) return rc;
  if ((rc = ensure(h, h->YT, (size_t)RHS_ROWS * ld * sizeof(T)))) return rc;
  if ((rc = ensure(h, h->Cneg, (size_t)RHS_ROWS * ld * sizeof(T)))) return rc;
  if ((rc = ensure(h, h->scalars, 64))) return rc;
  if ((rc = ensure(h, h->info, 64))) return rc;
  // Replicated-factor mode: every gathered panel passes through every rank, so a rank can
  // keep the WHOLE factor when it fits (34 GB at N = 65536) — then z = L^-1 y is a local
  // solve and predict splits the query points over the ranks with no per-panel exchange
  // (instead of broadcasting an nb x M block per panel).  Same decision on every rank: it
  // depends on N and the card's total memory only.  C4-sized problems (550 GB) stay
  // distributed.
  {
    size_t freeb = 0, totalb = 0;
    HIPCHK(h, hipMemGetInfo(&freeb, &totalb));
    h->repl = (double)(Npad + RHS_ROWS) * (double)ld * (double)sizeof(T) <= 0.35 * (double)totalb;
    if (env.shard_replicate >= 0) h->repl = env.shard_replicate != 0;
  }
  const bool repl = h->repl;
  // replicated factor + dense panel solves: every rank also keeps the explicit block inverses W_p that pass through it
  // with the diagonal blocks (N nb doubles: 0.5 GB at N = 65536, nb = 1024), for the streaming few-right-hand-side solver
  // and predict's dense block solves — what the unsharded handle has in Wblk
  const bool dense_panel = env.shard_dense_panel;
  const bool keep_w = repl && dense_panel;
  h->nbw = 0;  // valid again once this fit has finished
  if (keep_w && (rc = ensure(h, h->Wblk, (size_t)sh.nblk * nb * nb * sizeof(T)))) return rc;
  if (repl) {
    if ((rc = ensure(h, h->Lfull, (size_t)(Npad + RHS_ROWS) * ld * sizeof(T)))) return rc;
    h->Lfac = h->Lfull.p;
    h->zT = (T*)h->Lfull.p + Npad * ld;
    h->alphaT = nullptr;
    h->alpha_ready = false;
  } else {
    h->Lfac = nullptr;
    h->alphaT = h->YT.p;
    h->alpha_ready = true;
  }
  T* Lfull = repl ? (T*)h->Lfull.p : nullptr;
  T* A = (T*)h->K.p;
  T* Winv = (T*)h->Winv.p;
  T* PlocB[2] = {(T*)h->P.p, (T*)h->P.p + plocE};
  T* GB[2] = {(T*)h->G.p, (T*)h->G.p + gE};
  T* DbufB[2] = {(T*)h->Dbuf.p, (T*)h->Dbuf.p + dE};
  T* YTloc = (T*)h->YTloc.p;
  double* scal = (double*)h->scalars.p;  // [0] logdet partial, [1] info as double
  int* dInfo = (int*)h->info.p;
  hipStream_t st = h->st;
  const int tpb = nb / TILE;
  {
    PhaseScope total(h, &tm.fit_total);
    {
      PhaseScope ps(h, &tm.h2d);
      if ((rc = copy_in(h, h->X.p, X, (size_t)N * d * sizeof(T), mem_kind))) return rc;
      if ((rc = copy_in(h, h->Y.p, y, (size_t)N * k * sizeof(T), mem_kind))) return rc;
      if ((rc = copy_in(h, h->ls.p, lengthscale, (size_t)n_ls * 8, GPX_MEM_HOST))) return rc;
      const int init = INT_MAX;
      HIPCHK(h, hipMemcpyAsync(dInfo, &init, sizeof(int), hipMemcpyHostToDevice, st));
      HIPCHK(h, hipMemsetAsync(scal, 0, 64, st));
    }
    {
      // Every rank must have made the same choices — block height, dealing, problem size, riding query rows come from the
      // caller and the ENVIRONMENT of each rank's process — or the exchanges below move differently shaped pieces and the
      // result is silently wrong: one min-all-reduce of (x, -x) pairs before anything is exchanged; unequal -> every rank fails.
      double agree[6] = {(double)nb, -(double)nb, (double)(2 * N + sh.snake), -(double)(2 * N + sh.snake),
                         (double)(Xq ? Mquery : -1), -(double)(Xq ? Mquery : -1)};
      HIPCHK(h, hipMemcpyAsync(scal + 2, agree, sizeof(agree), hipMemcpyHostToDevice, st));
      {
        PhaseScope pc(h, &tm.comm);
        COMMCHK(cm->allreduce(h, scal + 2, 6, COMM_MIN));
      }
      HIPCHK(h, hipMemcpyAsync(agree, scal + 2, sizeof(agree), hipMemcpyDeviceToHost, st));
      HIPCHK(h, hipStreamSynchronize(st));
      if (agree[0] != -agree[1] || agree[2] != -agree[3] || agree[4] != -agree[5])
        return fail(h, GPX_E_ARG, "the ranks of the shard disagree on the block height, the dealing (GPX_NB_SHARD / GPX_SHARD_DEAL in "
                                  "each rank's environment), N or the query rows: nothing was exchanged");
    }
    {  // kernel build: own row blocks, columns up to and including the diagonal block
      PhaseScope ps(h, &tm.kbuild);
      const T* Xs = (const T*)h->Xs.p;
      launch_scale_points((const T*)h->X.p, N, Npad, d, (const double*)h->ls.p, n_ls,
                          (T*)h->Xs.p, st);
      for (int64_t lb = 0; lb < nlb; ++lb) {
        const int64_t g = sh.global(sh.r, lb);
        const int64_t mvalid = std::max<int64_t>(0, std::min<int64_t>(nb, N - g * nb));
        const int64_t ncols = (g + 1) * nb;
        launch_kbuild_cross(h->cfg.kernel, Xs + g * nb * d, mvalid, nb, Xs, std::min<int64_t>(N, ncols),
                            ncols, d, sf2, A + lb * nb * ld, ld, st);
        launch_fix_diag(A + lb * nb * ld + g * nb, ld, nb, (int)mvalid, sn2 + jitter, st);
      }
      if (Mq > 0) {  // bordered rows [nloc, nloc + Mq): K(Xq_r, X), every column
        if ((rc = upload_queries<T>(h, (const char*)Xq + (size_t)mq0 * d * sizeof(T), Mr, mem_kind))) return rc;
        launch_kbuild_cross(h->cfg.kernel, (const T*)h->scr.Qs.p, Mr, Mq, Xs, N, Npad, d, sf2, A + nloc * ld, ld, st);
      }
    }
    {
      // One-panel look-ahead, as on one GPU: the update of panel p is split into the STRIP
      // (the columns of block p+1) and the REST; stream s1 (high priority) then factors
      // diagonal block p+1 on its owner, broadcasts it, solves panel p+1 on every rank and
      // all-gathers it into the OTHER buffer set while s0 runs the rest of update p.
      PhaseScope ps(h, &tm.chol);
      hipStream_t s0 = h->st, s1 = h->st2;
      // panel(p, set, stream): diag + broadcast + local solve + all-gather + un-permute
      // Panel solve of every rank as ONE dense product with the block inverse W_p the owner builds
      // beside its diagonal chain and broadcasts with the block (default), or by the slab kernel
      // with the 64-block inverses.  The dense form takes ~0.2 ms of latency chain per panel off
      // the exchange path that bounds the factorisation at P = 8 (at the price of nb^2 more doubles
      // per broadcast); which one wins on real xGMI hardware is unmeasured (one-GPU rehearsals, where
      // the ranks hide each other's latency chains, favour the slab form by 5-25 %).
      // (GPX_SHARD_DENSE_PANEL: dense_panel above)
      hipEvent_t e_copied[2] = {nullptr, nullptr};  // copy-back of the panel last written into Ploc[set]
      hipEvent_t e_lcopy[2] = {nullptr, nullptr};   // replicated factor: the copy of the panel last gathered into GB[set]
      // Replicated factor: the gathered panel goes into the full copy on the COPY stream, beside the REST (HBM work beside
      // MFMA work) instead of in front of it on the main stream (GPX_REPL_COPY_SIDE=0: A/B)
      const bool side_copy = env.repl_copy_side;
      // TWO PIPELINES (round 4): the owner of the next diagonal block runs its update (STRIP_D) and the block's chain on a
      // stream of their own (sd), right behind ITS solve of the panel — beside the all-gather of that panel on s1 instead
      // of behind it.  Per panel the cycle solve -> all-gather -> STRIP_D -> diagonal chain -> broadcast -> solve becomes
      // solve -> max(all-gather [+ STRIP_B on the main stream], STRIP_D + chain + broadcast) -> solve: the all-gather leaves
      // the path that bounds the late panels of a many-GPU run.  Same kernels on the same operands: bit-identical.
      // Default: from 4 ranks on.  On ONE card it cannot pay (the "all-gather" of one rank is a local copy that then runs
      // beside the chain: fit 1393 -> 1400 ms; four ranks sharing the card: equal within noise — profiles/r04_two_pipelines.txt);
      // what it is worth over xGMI is the model's (tools/scaling_model.py), unmeasured.  GPX_SHARD_TWO_PIPE=0 / 1 forces it.
      const bool split_env = env.split_strip;  // (on a shard there is no fused strip; the two pipelines belong to the split schedule)
      const bool two_pipe = (env.shard_two_pipe >= 0 ? env.shard_two_pipe != 0 : sh.P >= 4) && split_env;
      if (two_pipe && !h->st5) {
        int lo = 0, hi = 0;
        HIPCHK(h, hipDeviceGetStreamPriorityRange(&lo, &hi));
        HIPCHK(h, hipStreamCreateWithPriority(&h->st5, hipStreamNonBlocking, hi));
      }
      hipStream_t sd = two_pipe ? h->st5 : s1;
      hipEvent_t e_solved[2] = {nullptr, nullptr};  // this rank's solve of the panel last written into Ploc[set]
      // before_solve (split schedule): what the local panel solve waits for — this rank's update of its own rows in
      // the panel's columns, which runs on the main stream beside the owner's diagonal chain and the broadcast
      auto panel = [&](int64_t p, int set, hipStream_t sx, hipEvent_t before_solve) -> int {
        const int64_t o = p * nb;
        const int root = sh.owner(p);
        const int64_t lo = sh.local(p) * nb;  // local row offset of block p on its owner
        T* Dbuf = DbufB[set];
        const bool last = p + 1 == sh.nblk;
        // W_p = L_pp^-1 is wanted by the panel below this block, and — replicated factor — by the streaming few-right-hand-
        // side solver (z-solve, alpha on demand) and the dense block solves of predict, which need it for EVERY block
        // (bordered query rows lie below every block; `ride` and not this rank's Mq: the broadcast is a collective, every
        //  rank must make the same decision also when its own slice of the query points is empty)
        const bool below = dense_panel && (!last || keep_w || ride);
        T* Wp = Dbuf + (int64_t)nb * nb + (int64_t)nb * KB;
        // the owner's chain: on its own stream beside the previous panel's all-gather (two pipelines), except for panel 0
        hipStream_t sdx = (two_pipe && p > 0 && sx == s1) ? sd : sx;
        if (sh.r == root) {
          PhaseScope pd(h, &tm.chol_diag, profile, sdx);
          T* Ablk = A + lo * ld + o;
          // the explicit inverse W_p = L_pp^-1 is built beside the diagonal chain (side stream)
          // straight into the broadcast buffer: every rank's panel solve is then one dense product
          InvWork<T> iw;
          iw.W = Wp;
          iw.U = (T*)h->Ublk.p;
          iw.ldu = ldp;
          iw.nbw = nb;
          iw.aux = h->st3;
          COMMCHK(diag_enqueue<T>(h, Ablk, ld, 0, nb, Winv + (o / KB) * (KB * KB), dInfo, o, sdx,
                                       below ? &iw : nullptr));
          launch_logdet_acc(Ablk, ld, nb, scal, sdx);
          HIPCHK(h, hipMemcpy2DAsync(Dbuf, (size_t)nb * sizeof(T), Ablk, (size_t)ld * sizeof(T), (size_t)nb * sizeof(T), nb,
                                     hipMemcpyDeviceToDevice, sdx));
          HIPCHK(h, hipMemcpyAsync(Dbuf + (int64_t)nb * nb, Winv + (o / KB) * (KB * KB),
                                   (size_t)nb * KB * sizeof(T), hipMemcpyDeviceToDevice, sdx));
          if (below) HIPCHK(h, hipStreamWaitEvent(sdx, iw.ready, 0));
          if (sdx != sx) {  // the block joins the exchange stream in front of its broadcast
            COMMCHK(stream_waits(h, sx, sdx, "diagonal chain"));
          }
        }
        if (last && !repl && !ride) return GPX_OK;  // last block: nothing below it
        {
          PhaseScope pc(h, &tm.comm, true, sx);
          COMMCHK(cm->bcast(h, Dbuf, (size_t)nb * nb + (size_t)nb * KB + (below ? (size_t)nb * nb : 0), root, sx));
        }
        if (repl) {  // keep L_pp and the inverses of its 64-blocks
          HIPCHK(h, hipMemcpy2DAsync(Lfull + o * ld + o, (size_t)ld * sizeof(T), Dbuf, (size_t)nb * sizeof(T), (size_t)nb * sizeof(T), nb,
                                     hipMemcpyDeviceToDevice, sx));
          if (sh.r != root)
            HIPCHK(h, hipMemcpyAsync(Winv + (o / KB) * (KB * KB), Dbuf + (int64_t)nb * nb, (size_t)nb * KB * sizeof(T),
                                     hipMemcpyDeviceToDevice, sx));
          if (keep_w)
            HIPCHK(h, hipMemcpyAsync((T*)h->Wblk.p + p * (int64_t)nb * nb, Wp, (size_t)nb * nb * sizeof(T),
                                     hipMemcpyDeviceToDevice, sx));
          if (last && !ride) return GPX_OK;
        }
        if (before_solve) HIPCHK(h, hipStreamWaitEvent(sx, before_solve, 0));
        const int64_t lb0 = sh.lb0(p, sh.r);
        const int64_t rows = nloc - lb0 * nb + Mq;  // own trailing rows + the bordered query rows right behind them
        if (rows > 0 && !dense_panel) {  // the slab kernel with the 64-block inverses (GPX_SHARD_DENSE_PANEL=0)
          PhaseScope pt(h, &tm.chol_trsm, profile, sx);
          launch_trsm_rlt<T>(A + lb0 * nb * ld + o, ld, rows, Dbuf, nb, Dbuf + (int64_t)nb * nb, nb,
                                  PlocB[set], ldp, sx);
        } else if (rows > 0) {  // own rows of the panel: P = A_rows W_p^T (compact), copied back into A beside the update
          PhaseScope pt(h, &tm.chol_trsm, profile, sx);
          T* Arows = A + lb0 * nb * ld + o;
          if (e_copied[set]) HIPCHK(h, hipStreamWaitEvent(sx, e_copied[set], 0));  // Ploc[set] is free again
          launch_gemm_nt<T>(128, PlocB[set], ldp, Arows, ld, Wp, nb, rows, nb, nb, 4, 1, sx);
          COMMCHK(stream_waits(h, h->st4, sx, "panel copy"));
          launch_copy2d<T>(Arows, ld, PlocB[set], ldp, rows, nb, h->st4);
          COMMCHK(record_event(h, h->st4, "panel copy", &e_copied[set]));
        }
        // "this rank's rows of panel p are solved" — what the next diagonal block's update waits for
        if (two_pipe) COMMCHK(record_event(h, sx, "panel solve", &e_solved[set]));
        if (last) return GPX_OK;  // (only bordered rows below the last block: nobody's operand)
        const int64_t mc = sh.maxcnt(p);
        if (e_lcopy[set]) HIPCHK(h, hipStreamWaitEvent(sx, e_lcopy[set], 0));  // GB[set] is free again
        {
          PhaseScope pc(h, &tm.comm, true, sx);
          COMMCHK(cm->allgather(h, PlocB[set], GB[set], (size_t)mc * ldp, sx));
        }
        // (no un-permute, round 4: the update kernels read the gathered panel in place — bc_brow in gpx_tile.h — and the
        //  replicated factor's column block is written from it off the chain, on the main stream)
        return GPX_OK;
      };
      // Schedule (round 4: the single-GPU split schedule of chol_enqueue, DESIGN.md §3.2 item 3, on every rank).  Per panel p:
      //   look-ahead stream s1, the CHAIN: [owner of block p+1] update of that DIAGONAL block only (STRIP_D: its operand
      //     is the owner's own rows of the solved panel p — no exchange, right behind the un-permute that completed it),
      //     diagonal block p+1, then on every rank: broadcast -> [wait e_below(p)] -> solve of the own rows of panel p+1
      //     -> all-gather -> un-permute -> e_panel(p+1).
      //   main stream s0, THROUGHPUT: STRIP_B(p) = own rows below block p+1 in its columns (dense) -> e_below(p) ->
      //     [replicated factor: panel p into the full copy] -> REST(p) -> e_main(p) -> wait e_panel(p+1).  Where the chain
      //     sets the pace (REST small) the REST hands its first column block (that of panel p+2, incl. diagonal block p+2)
      //     over as a launch of its own: REST_A -> e_main(p) -> REST_B, so that the next STRIP_D never waits for the bulk.
      // Round 3 ran the whole STRIP on the main stream first and started the chain behind it (GPX_SPLIT_STRIP=0 keeps that
      // form: A/B and bit-identity tests): a step was STRIP + max(REST, chain); now it is max(STRIP_B + REST, chain).
      const int rest_split = env.rest_split;  // as chol_enqueue: trailing rows (in panels, per sqrt(P)) up to which the REST is split
      // first row of block g (> q) in the gathered panel q: rank-major pieces of maxcnt(q) rows, each rank's own blocks
      // beyond q in order (what bc_brow computes per tile column inside the staircase kernel)
      auto grow = [&](int64_t q, int64_t g) -> int64_t {
        const int rr = sh.owner(g);
        return (int64_t)rr * sh.maxcnt(q) + (sh.local(g) - sh.lb0(q, rr)) * nb;
      };
      COMMCHK(panel(0, 0, s0, nullptr));
      hipEvent_t e_main = nullptr;  // "this rank's updates of the trailing matrix that touch the next diagonal block are complete"
      if (split_env && sh.nblk > 1) COMMCHK(record_event(h, s0, "look-ahead", &e_main));
      for (int64_t p = 0; p + 1 < sh.nblk; ++p) {
        const int cur = (int)(p & 1), nxt = cur ^ 1;
        const int64_t lb0 = sh.lb0(p, sh.r), rows = nloc - lb0 * nb;
        const int64_t lb1 = sh.lb0(p + 1, sh.r), rows1 = nloc - lb1 * nb;
        const int64_t ntrail = (sh.nblk - p - 1) * nb, nrest = ntrail - nb;
        const int64_t mcp = sh.maxcnt(p);  // rows per rank piece of the gathered panel p (GB[cur])
        hipEvent_t e_panel = next_event(h);
        if (!e_panel) return fail(h, GPX_E_HIP, "hipEventCreate failed (look-ahead)");
        if (split_env) {
          const bool own_next = sh.owner(p + 1) == sh.r;  // then local block lb0 IS block p+1 (rows [0, nb) of Ploc[cur])
          if (own_next) {  // STRIP_D: the next diagonal block, lower triangle, on the chain
            HIPCHK(h, hipStreamWaitEvent(sd, e_main, 0));  // the previous REST (its first column block) touched the block
            // two pipelines: behind this rank's solve of panel p (and with it everything older on s1), not behind the all-gather
            if (sd != s1 && e_solved[cur]) HIPCHK(h, hipStreamWaitEvent(sd, e_solved[cur], 0));
            PhaseScope pu(h, &tm.chol_strip, profile, sd);
            launch_gemm_nt<T>(128, A + lb0 * nb * ld + (p + 1) * nb, ld, PlocB[cur], ldp, PlocB[cur], ldp, nb, nb, nb, 1, 0,
                                   sd);
          }
          // the host enqueues the main stream's whole iteration BEFORE the chain's dozens of small launches
          if (rows1 + Mq > 0) {  // STRIP_B: own rows below block p+1 (and the bordered rows) x its columns (every tile)
            PhaseScope pu(h, &tm.chol_strip, profile);
            launch_gemm_nt<T>(128, A + lb1 * nb * ld + (p + 1) * nb, ld, PlocB[cur] + (lb1 - lb0) * nb * ldp, ldp,
                                   GB[cur] + grow(p, p + 1) * ldp, ldp, rows1 + Mq, (int64_t)nb, nb, 0, 0, s0);
          }
          hipEvent_t e_below;
          COMMCHK(record_event(h, s0, "look-ahead", &e_below));
          if (repl) {  // panel p into the full factor (un-permuted on the way): off the panel chain
            hipStream_t sc = side_copy ? h->st4 : s0;
            if (side_copy) HIPCHK(h, hipStreamWaitEvent(sc, e_below, 0));  // (s0 waited for the gathered panel p before)
            launch_unpermute_panel(GB[cur], ldp, Lfull + (p + 1) * nb * ld + p * nb, ld, nb, sh.deal(), (int)p, (int)sh.nblk, mcp, sc);
            if (side_copy) COMMCHK(record_event(h, sc, "panel copy", &e_lcopy[cur]));
          }
          // REST: own rows beyond block p+1 x columns beyond it (block-cyclic staircase).  The panel buffers it reads are
          // rewritten two panel solves later, behind e_below(p+1) of this stream, i.e. behind all of this update.
          const bool ahead = nrest > nb && (double)nrest <= (double)rest_split * nb * std::sqrt((double)sh.P);
          // (the bordered rows ride in these launches: local tile rows beyond the own blocks stand for blocks beyond the
          //  matrix, so the staircase gives them every column)
          if (ahead && rows1 + Mq > 0) {  // REST_A: the column block of panel p+2 (own rows from block p+2 on)
            PhaseScope pu(h, &tm.chol_strip, profile);
            launch_gemm_nt_bc(A + lb1 * nb * ld + (p + 2) * nb, ld, PlocB[cur] + (lb1 - lb0) * nb * ldp, ldp,
                              GB[cur], ldp, rows1 + Mq, (int64_t)nb, nb, sh.mask(tpb, lb1, p + 2, p, mcp), s0);
          }
          if (ahead) COMMCHK(record_event(h, s0, "look-ahead", &e_main));
          if (ahead) {  // REST_B: own rows beyond block p+2 x columns beyond it
            const int64_t lb2 = sh.lb0(p + 2, sh.r), rows2 = nloc - lb2 * nb;
            if (rows2 + Mq > 0 && nrest - nb > 0) {
              PhaseScope pu(h, &tm.chol_syrk, profile);
              launch_gemm_nt_bc(A + lb2 * nb * ld + (p + 3) * nb, ld, PlocB[cur] + (lb2 - lb0) * nb * ldp, ldp,
                                GB[cur], ldp, rows2 + Mq, nrest - nb, nb, sh.mask(tpb, lb2, p + 3, p, mcp), s0);
              tm.syrk_launches += 1;
            }
          } else {
            if (rows1 + Mq > 0 && nrest > 0) {
              PhaseScope pu(h, &tm.chol_syrk, profile);
              launch_gemm_nt_bc(A + lb1 * nb * ld + (p + 2) * nb, ld, PlocB[cur] + (lb1 - lb0) * nb * ldp, ldp,
                                GB[cur], ldp, rows1 + Mq, nrest, nb, sh.mask(tpb, lb1, p + 2, p, mcp), s0);
              tm.syrk_launches += 1;
            }
            COMMCHK(record_event(h, s0, "look-ahead", &e_main));
          }
          COMMCHK(panel(p + 1, nxt, s1, e_below));
          HIPCHK(h, hipEventRecord(e_panel, s1));
          HIPCHK(h, hipStreamWaitEvent(s0, e_panel, 0));
          continue;
        }
        if (ride) return fail(h, GPX_E_UNSUPPORTED, "query rows ride only in the split schedule of the sharded factorisation");
        if (rows > 0) {  // STRIP: own trailing rows x block column p+1
          PhaseScope pu(h, &tm.chol_strip, profile);
          launch_gemm_nt_bc(A + lb0 * nb * ld + (p + 1) * nb, ld, PlocB[cur], ldp, GB[cur], ldp, rows,
                            (int64_t)nb, nb, sh.mask(tpb, lb0, p + 1, p, mcp), s0);
        }
        COMMCHK(stream_waits(h, s1, s0, "look-ahead"));
        if (repl)  // panel p into the full factor: behind the strip, i.e. off the panel chain
          launch_unpermute_panel(GB[cur], ldp, Lfull + (p + 1) * nb * ld + p * nb, ld, nb, sh.deal(), (int)p, (int)sh.nblk, mcp, s0);
        // the host enqueues the REST before the look-ahead chain's dozens of small launches (round 3, as on one
        // GPU: an update enqueued behind the chain reaches the GPU late when the chain runs as fast as it is enqueued)
        if (rows1 > 0 && nrest > 0) {  // REST: own rows beyond block p+1 x columns beyond it
          PhaseScope pu(h, &tm.chol_syrk, profile);
          launch_gemm_nt_bc(A + lb1 * nb * ld + (p + 2) * nb, ld, PlocB[cur] + (lb1 - lb0) * nb * ldp, ldp,
                            GB[cur], ldp, rows1, nrest, nb, sh.mask(tpb, lb1, p + 2, p, mcp), s0);
          tm.syrk_launches += 1;
        }
        COMMCHK(panel(p + 1, nxt, s1, nullptr));
        HIPCHK(h, hipEventRecord(e_panel, s1));
        HIPCHK(h, hipStreamWaitEvent(s0, e_panel, 0));
      }
    }
    for (hipStream_t sj : {h->st3, h->st4, h->st5}) {  // every panel copy-back is in A before anything reads L from it
      if (sj) COMMCHK(stream_waits(h, st, sj, "join"));
    }
    if (!repl) {  // alpha = L^-T L^-1 y on the local column layout YTloc (64 x nloc), then replicated in the global layout
      PhaseScope ps(h, &tm.solve);
      launch_pack_rhs_local((const T*)h->Y.p, N, k, YTloc, ldy, nb, (int)nlb, sh.deal(), sh.r, RHS_ROWS, st);
      COMMCHK(shard_solve_dist<T>(h, sh, YTloc, (T*)h->YT.p, Xq ? &h->AT : nullptr));
      if (Xq) h->zT = h->AT.p;  // z^T = (L^-1 y)^T replicated: the fused predict's mean is V^T z
    } else {  // whole factor on every rank: z = L^-1 y locally (alpha on demand, as unsharded)
      PhaseScope ps(h, &tm.solve);
      T* zT = (T*)h->zT;
      launch_pack_rhs<T>((const T*)h->Y.p, N, k, zT, ld, Npad, (int)RHS_ROWS, st);
      h->nbw = keep_w ? nb : 0;  // the block inverses of this fit are complete on this rank (joined above: st3, and s1 through e_panel)
      // predict's block solves are dense products with them when its block width is theirs: follow the shard's block
      // (512 query rows per rank at nb = 512, P = 8: 46.5 ms dense against 52.8 ms with 1024-wide slab solves — profiles/r04_predict_block_ab.txt)
      if (keep_w && env.nb_pred < 0) h->nb_pred = nb;
      if (few_solver_applies(h)) {  // k <= 8: one stream over the factor with the block inverses (round 4; 18 ms -> ~2 at N = 65536)
        if ((rc = solve_few<T>(h, zT, k, Lfull, ld, Npad, (const T*)h->Wblk.p, nb, true, false))) return rc;
      } else if ((rc = solve_fwd_enqueue<T>(h, zT, RHS_ROWS, Lfull, ld, Npad, h->nb_solve, Winv))) {
        return rc;
      }
    }
    {
      PhaseScope ps(h, &tm.logdet);
      PhaseScope pc(h, &tm.comm);
      COMMCHK(cm->allreduce(h, scal, 1, COMM_SUM));
    }
  }
  int hinfo = 0;
  HIPCHK(h, hipMemcpyAsync(&hinfo, dInfo, sizeof(int), hipMemcpyDeviceToHost, st));
  HIPCHK(h, hipMemcpyAsync(&h->logdet, scal, sizeof(double), hipMemcpyDeviceToHost, st));
  HIPCHK(h, hipStreamSynchronize(st));
  // First bad pivot over all ranks.  A parked stream that timed out on ANY rank (INT_MIN in its info word) survives the
  // min as well, so every rank learns of it here and they leave — or retry — TOGETHER: a rank returning before this
  // collective would leave its peers blocked in it (ADVICE r3).
  double dinfo = (hinfo == INT_MAX) ? 1e300 : (double)hinfo;
  HIPCHK(h, hipMemcpyAsync(scal + 1, &dinfo, sizeof(double), hipMemcpyHostToDevice, st));
  COMMCHK(cm->allreduce(h, scal + 1, 1, COMM_MIN));
  HIPCHK(h, hipMemcpyAsync(&dinfo, scal + 1, sizeof(double), hipMemcpyDeviceToHost, st));
  if ((rc = finish_call(h))) return rc;
  if (dinfo < 0) {  // same decision on every rank: dinfo is all-reduced, the environment is the launch's (retry_with_events uses nothing rank-local)
    if (retry_with_events(h, retried))  // this handle hands over by hipEvents from now on; the fit runs once more (same kernels, same bits)
      return shard_fit<T>(h, X, y, N, d, k, lengthscale, n_ls, sf2, sn2, jitter, mem_kind, info, true, Xq, Mquery);
    return fail(h, GPX_E_HIP, "a stream parked on a device flag timed out on some rank (kernels serialised across streams? set GPX_CHAIN_FLAG=0)");
  }
  tm.handover_flags = chain_flag_enabled(h) ? 1.0 : 0.0;
  tm.handover_retries = (double)h->flag_retries;
  *info = dinfo >= 1e299 ? 0 : (int64_t)dinfo;
  h->fitted = (*info == 0);
  return GPX_OK;
}

// Every rank holds the posterior of ITS slice of the query points (rows [r Mc, (r + 1) Mc) of M: h->meanout (Mr x k),
// h->var (Mr)): one all-gather of (mean | var) slices, then the whole result on every rank (rank 0 of a group delivers).
template <typename T>
int shard_gather_slices(gpx_handle* h, int64_t M, int64_t Mc, int64_t Mr, bool want_var, void* mean, void* var,
                        int32_t mem_kind) {
  Comm* cm = h->comm;
  const int P = cm->world;
  const int k = h->k;
  const size_t slot = (size_t)Mc * (k + 1);  // elements per rank: mean (Mc x k) then var (Mc)
  gpx_timings& tm = h->tm;
  int rc;
  if ((rc = ensure(h, h->scr.GatherS, slot * sizeof(T)))) return rc;
  if ((rc = ensure(h, h->scr.GatherR, slot * 8 * P))) return rc;
  if ((rc = ensure(h, h->scr.outM, (size_t)M * k * sizeof(T)))) return rc;
  if ((rc = ensure(h, h->scr.outV, (size_t)M * sizeof(T)))) return rc;
  T* S = (T*)h->scr.GatherS.p;
  T* R = (T*)h->scr.GatherR.p;
  hipStream_t st = h->st;
  HIPCHK(h, hipMemsetAsync(S, 0, slot * sizeof(T), st));
  if (Mr > 0) {
    HIPCHK(h, hipMemcpyAsync(S, h->meanout.p, (size_t)Mr * k * sizeof(T), hipMemcpyDeviceToDevice, st));
    if (want_var)
      HIPCHK(h, hipMemcpyAsync(S + (size_t)Mc * k, h->var.p, (size_t)Mr * sizeof(T), hipMemcpyDeviceToDevice, st));
  }
  {
    PhaseScope pc(h, &tm.comm);
    COMMCHK(cm->allgather(h, S, R, slot));
  }
  for (int q = 0; q < P; ++q) {
    const int64_t q0 = std::min<int64_t>(M, (int64_t)q * Mc), q1 = std::min<int64_t>(M, (int64_t)(q + 1) * Mc);
    if (q1 <= q0) continue;
    HIPCHK(h, hipMemcpyAsync((T*)h->scr.outM.p + q0 * k, R + (size_t)q * slot, (size_t)(q1 - q0) * k * sizeof(T),
                             hipMemcpyDeviceToDevice, st));
    if (want_var)
      HIPCHK(h, hipMemcpyAsync((T*)h->scr.outV.p + q0, R + (size_t)q * slot + (size_t)Mc * k,
                               (size_t)(q1 - q0) * sizeof(T), hipMemcpyDeviceToDevice, st));
  }
  PhaseScope ps(h, &tm.d2h);
  if (!h->discard_out) {  // a group's ranks > 0 hold the same result; rank 0 delivers it
    if ((rc = copy_out(h, mean, h->scr.outM.p, (size_t)M * k * sizeof(T), mem_kind))) return rc;
    if (want_var && (rc = copy_out(h, var, h->scr.outV.p, (size_t)M * sizeof(T), mem_kind))) return rc;
  }
  return GPX_OK;
}

// The predict half of gpx_fit_predict on a shard: V^T of this rank's slice of the query points sits in the bordered rows
// [nloc, nloc + fq_rows) of its K buffer (shard_fit with query points), z^T replicated in h->zT: the mean V^T z, the row
// norms, one all-gather of the slices.  Collective: every rank calls it (a rank whose slice is empty only gathers).
template <typename T>
int shard_fused_tail(gpx_handle* h, int64_t M, void* mean, void* var, int32_t mem_kind) {
  Comm* cm = h->comm;
  const int P = cm->world, r = cm->rank;
  const int64_t Mc = round_up((M + P - 1) / P, TILE);
  const int64_t m0 = std::min<int64_t>(M, (int64_t)r * Mc), m1 = std::min<int64_t>(M, (int64_t)(r + 1) * Mc);
  const int64_t Mr = m1 - m0, Mq = round_up(Mr, TILE), ldm = Mq + ld_skew<T>();
  if (Mq != h->fq_rows) return fail(h, GPX_E_ARG, "gpx_fit_predict: the factorisation carried other query rows");
  reset_predict_clocks(h->tm);
  int rc;
  if ((rc = ensure(h, h->meanout, (size_t)std::max<int64_t>(Mr, 1) * h->k * sizeof(T)))) return rc;
  if ((rc = ensure(h, h->var, (size_t)std::max<int64_t>(Mq, TILE) * sizeof(T)))) return rc;
  {
    PhaseScope total(h, &h->tm.predict_total);
    if (Mr > 0) {
      if ((rc = ensure(h, h->scr.MT, (size_t)RHS_ROWS * ldm * sizeof(T)))) return rc;
      if ((rc = ensure_mean_partials<T>(h, h->scr.MTpart, ldm))) return rc;
      bordered_mean_var<T>(h, (const T*)h->K.p + h->nloc * h->ld, Mr, Mq, ldm, var != nullptr);
    }
    if ((rc = shard_gather_slices<T>(h, M, Mc, Mr, var != nullptr, mean, var, mem_kind))) return rc;
  }
  return finish_call(h);
}

// Replicated-factor predict: rank r takes query points [r*Mc, (r+1)*Mc) through the
// single-GPU path (predict_core, whole L), then one all-gather of (mean | var) slices.
template <typename T>
int shard_predict_repl(gpx_handle* h, const void* Xq, int64_t M, void* mean, void* var, int32_t mem_kind) {
  Comm* cm = h->comm;
  const int P = cm->world, r = cm->rank;
  const int d = h->d;
  const int64_t Mc = round_up((M + P - 1) / P, TILE);
  const int64_t m0 = std::min<int64_t>(M, (int64_t)r * Mc), m1 = std::min<int64_t>(M, (int64_t)(r + 1) * Mc);
  const int64_t Mr = m1 - m0;
  reset_predict_clocks(h->tm);
  int rc;
  {
    PhaseScope total(h, &h->tm.predict_total);
    if ((rc = predict_core<T>(h, (const char*)Xq + (size_t)m0 * d * sizeof(T), Mr, var != nullptr, mem_kind)))
      return rc;
    if ((rc = shard_gather_slices<T>(h, M, Mc, Mr, var != nullptr, mean, var, mem_kind))) return rc;
  }
  return finish_call(h);
}

// XT (mp rows x own columns, ldv) <- XT L^-T over the block-cyclic column layout (local column block lb =
// global block lb P + r), column blocks p >= p0 (everything left of block p0 is known to be zero), with
// one-block look-ahead as in the factorisation: the update of block p is split into the STRIP (the
// columns of block p+1, on the rank that owns them) and the REST; the look-ahead stream then solves
// block p+1 on its owner and broadcasts it (into the other Sv buffer) while the main stream runs the
// rest of update p on every rank.  Every rank must call it with the same mp and p0 (collectives inside).
template <typename T>
int shard_fwd_sweep(gpx_handle* h, const Shard& sh, T* VT, int64_t ldv, int64_t mp, int64_t p0, T* const SvB[2]) {
  Comm* cm = h->comm;
  const int nb = sh.nb;
  const int64_t ld = h->ld, nloc = h->nloc;
  const T* A = (const T*)h->K.p;
  const T* Winv = (const T*)h->Winv.p;
  gpx_timings& tm = h->tm;
  hipStream_t st = h->st, s1 = h->st2;
  auto solve_block = [&](int64_t p, int set, hipStream_t sx) -> int {  // owner solves + everybody receives
    const int64_t o = p * nb, lo = sh.local(p) * nb;
    const int root = sh.owner(p);
    if (sh.r == root) {
      launch_trsm_rlt<T>(VT + lo, ldv, mp, A + lo * ld + o, ld, Winv + (o / KB) * (KB * KB), nb,
                              nullptr, 0, sx);
      if (p + 1 < sh.nblk)
        HIPCHK(h, hipMemcpy2DAsync(SvB[set], (size_t)nb * sizeof(T), VT + lo, (size_t)ldv * sizeof(T), (size_t)nb * sizeof(T),
                                   (size_t)mp, hipMemcpyDeviceToDevice, sx));
    }
    if (p + 1 == sh.nblk) return GPX_OK;
    PhaseScope pc(h, &tm.comm, true, sx);
    return cm->bcast(h, SvB[set], (size_t)mp * nb, root, sx);
  };
  if (p0 >= sh.nblk) return GPX_OK;
  const int tile = mp % 128 == 0 ? 128 : 64;  // mp = 64: the right-hand sides of the fit (one MFMA slab)
  COMMCHK(solve_block(p0, 0, st));
  for (int64_t p = p0; p + 1 < sh.nblk; ++p) {
    const int cur = (int)((p - p0) & 1), nxt = cur ^ 1;
    const int64_t o = p * nb;
    const int64_t lb0 = sh.lb0(p, sh.r), rows = nloc - lb0 * nb;   // own columns beyond block p
    const bool own_next = sh.owner(p + 1) == sh.r;                 // then local block lb0 is block p+1
    if (own_next)  // STRIP
      launch_gemm_nt(tile, VT + lb0 * nb, ldv, SvB[cur], nb, A + lb0 * nb * ld + o, ld, mp, (int64_t)nb, nb, 0,
                     0, st);
    hipEvent_t e_strip = next_event(h), e_blk = next_event(h);
    if (!e_strip || !e_blk) return fail(h, GPX_E_HIP, "hipEventCreate failed (look-ahead)");
    HIPCHK(h, hipEventRecord(e_strip, st));
    HIPCHK(h, hipStreamWaitEvent(s1, e_strip, 0));
    COMMCHK(solve_block(p + 1, nxt, s1));
    HIPCHK(h, hipEventRecord(e_blk, s1));
    const int64_t skip = own_next ? nb : 0;
    if (rows - skip > 0)  // REST
      launch_gemm_nt(tile, VT + lb0 * nb + skip, ldv, SvB[cur], nb, A + (lb0 * nb + skip) * ld + o, ld, mp,
                     rows - skip, nb, 0, 0, st);
    HIPCHK(h, hipStreamWaitEvent(st, e_blk, 0));
  }
  return GPX_OK;
}

// Gradient of the log marginal likelihood when the factor is ONLY held distributed (C4-sized problems:
// no rank can hold L, let alone L^-T).  K^-1 = L^-T L^-1 = sum_k ZT[:, k] ZT[:, k]^T, and the trace with
// dK/dtheta is linear in it, so the contraction index k is what gets distributed:
//   1. ZTc = the columns of ZT = L^-T that belong to this rank's row blocks of L, for ALL rows: the
//      distributed forward substitution of the variance path (shard_fwd_sweep) on the identity, in row
//      batches, skipping the column blocks left of a batch (structural zeros): N^3 / (3 P) flops per
//      rank, one (batch x nb) broadcast per block step — the lower triangle once, as in the factorisation;
//      memory N^2 / P, the size of the rank's share of the factor.
//   2. the fused K^-1 trace kernel over EVERY tile, contracting over the own columns only (another
//      N^3 / (3 P) flops); 3. one all-reduce of the ntheta sums.
// alpha is already replicated (the fit solved it); its quadratic form is replicated O(N^2 k) work.
int shard_lml_grad_dist(gpx_handle* h, double* lml, double* grad) {
  Comm* cm = h->comm;
  const int nb = h->nb_shard;
  Shard sh{cm->world, cm->rank, nb, h->Npad / nb, h->shard_snake};
  const int64_t N = h->N, Npad = h->Npad, ld = h->ld, nloc = h->nloc;
  const int64_t nlb = sh.nlb(sh.r);
  const int d = h->d, k = h->k, ntheta = h->n_ls + 2, ard = h->n_ls > 1;
  const int64_t ldv = std::max<int64_t>(nloc, nb) + LD_SKEW;
  int64_t MB = pred_batch_rows(h, Npad, (size_t)ldv * 8, false) / nb * nb;   // whole blocks per batch: same on every rank
  if (MB < nb) MB = nb;
  gpx_timings& tm = h->tm;
  tm.grad_trtri = tm.grad_trace = tm.grad_total = 0;
  const int64_t s1n = kinv_trace_slots(Npad), s2n = alpha_quad_slots(Npad);
  int rc;
  if ((rc = ensure(h, h->scr.ZTloc, (size_t)Npad * ldv * 8))) return rc;
  if ((rc = ensure(h, h->scr.Sv, (size_t)2 * MB * nb * 8))) return rc;
  if ((rc = ensure(h, h->scr.gpart, (size_t)((s1n + s2n) * ntheta + 2 * ntheta + 1) * 8))) return rc;
  double* Z = (double*)h->scr.ZTloc.p;
  double* SvB[2] = {(double*)h->scr.Sv.p, (double*)h->scr.Sv.p + (size_t)MB * nb};
  double* part1 = (double*)h->scr.gpart.p;
  double* part2 = part1 + s1n * ntheta;
  double* outv = part2 + s2n * ntheta;
  hipStream_t st = h->st;
  {
    PhaseScope total(h, &tm.grad_total);
    {
      PhaseScope ps(h, &tm.grad_trtri);
      HIPCHK(h, hipMemsetAsync(Z, 0, (size_t)Npad * ldv * 8, st));
      for (int64_t lb = 0; lb < nlb; ++lb) {  // the identity in the own columns
        const int64_t g = sh.global(sh.r, lb);
        launch_set_diag_one(Z + g * nb * ldv + lb * nb, ldv, nb, st);
      }
      for (int64_t m0 = 0; m0 < Npad; m0 += MB) {
        const int64_t mp = std::min(MB, Npad - m0);
        if ((rc = shard_fwd_sweep(h, sh, Z + m0 * ldv, ldv, mp, m0 / nb, SvB))) return rc;
      }
    }
    {
      PhaseScope ps(h, &tm.grad_trace);
      HIPCHK(h, hipMemsetAsync(part1, 0, (size_t)(s1n + s2n) * ntheta * 8, st));
      if (nloc > 0)
        launch_kinv_trace_cols(h->cfg.kernel, Z, ldv, Npad, N, (const double*)h->Xs.p, d, ard, h->sf2, h->sn2, part1,
                               ntheta, nb, sh.P, sh.r, nloc, sh.snake, st);
    }
    launch_alpha_quad(h->cfg.kernel, (const double*)h->alphaT, ld, k, Npad, N, (const double*)h->Xs.p, d, ard,
                      h->sf2, h->sn2, part2, ntheta, st);
    launch_reduce_partials(part1, s1n, ntheta, 1.0, outv, st);
    launch_reduce_partials(part2, s2n, ntheta, 1.0, outv + ntheta, st);
    launch_dot_rhs((const double*)h->Y.p, (const double*)h->alphaT, ld, N, k, outv + 2 * ntheta, st);
    if ((rc = cm->allreduce(h, outv, (size_t)ntheta, COMM_SUM))) return rc;
  }
  double host[2 * 34 + 1];
  HIPCHK(h, hipMemcpyAsync(host, outv, (size_t)(2 * ntheta + 1) * 8, hipMemcpyDeviceToHost, st));
  if ((rc = finish_call(h))) return rc;
  for (int t = 0; t < ntheta; ++t) grad[t] = 0.5 * (host[ntheta + t] - (double)k * host[t]);
  *lml = -0.5 * host[2 * ntheta] - 0.5 * (double)k * h->logdet -
         0.5 * (double)N * (double)k * 1.8378770664093454835606594728112;  // log(2 pi)
  return GPX_OK;
}

template <typename T>
int shard_predict(gpx_handle* h, const void* Xq, int64_t M, void* mean, void* var, int32_t mem_kind) {
  if (h->repl) return shard_predict_repl<T>(h, Xq, M, mean, var, mem_kind);
  Comm* cm = h->comm;
  const int nb = h->nb_shard;
  Shard sh{cm->world, cm->rank, nb, h->Npad / nb, h->shard_snake};
  const int64_t N = h->N, nloc = h->nloc, ldy = h->ldy;
  const int64_t nlb = sh.nlb(sh.r);
  const int d = h->d, k = h->k;
  const int64_t Mpad = round_up(M, TILE);
  const int64_t ldm = Mpad + ld_skew<T>(), ldv = nloc + ld_skew<T>();
  // Query points go through in batches of MB rows (one V^T / broadcast buffer, memory
  // O(MB * N / P)); every rank must take the same batches — there are collectives inside the
  // loop — so the batch size depends on nothing but M and GPX_PRED_BATCH.
  const int64_t MB = pred_batch_rows(h, Mpad, (size_t)ldv * sizeof(T), false);
  gpx_timings& tm = h->tm;
  reset_predict_clocks(tm);
  int rc;
  if ((rc = ensure_queries<T>(h, M))) return rc;
  if ((rc = ensure(h, h->scr.VT, (size_t)MB * ldv * sizeof(T)))) return rc;
  if ((rc = ensure(h, h->scr.MT, (size_t)RHS_ROWS * ldm * sizeof(T)))) return rc;
  if ((rc = ensure(h, h->meanout, (size_t)M * k * sizeof(T)))) return rc;
  if ((rc = ensure(h, h->var, (size_t)Mpad * sizeof(T)))) return rc;
  if ((rc = ensure(h, h->scr.Sv, (size_t)2 * MB * nb * sizeof(T)))) return rc;
  T* VT = (T*)h->scr.VT.p;
  T* SvB[2] = {(T*)h->scr.Sv.p, (T*)h->scr.Sv.p + (size_t)MB * nb};
  const T* Xs = (const T*)h->Xs.p;
  hipStream_t st = h->st;
  {
    PhaseScope total(h, &tm.predict_total);
    {
      PhaseScope ps(h, &tm.kstar);
      if ((rc = upload_queries<T>(h, Xq, M, mem_kind))) return rc;
    }
    for (int64_t m0 = 0; m0 < Mpad; m0 += MB) {
      const int64_t mp = std::min(MB, Mpad - m0), mv = std::min<int64_t>(mp, M - m0);
      {
        PhaseScope ps(h, &tm.kstar);
        for (int64_t lb = 0; lb < nlb; ++lb) {
          const int64_t g = sh.global(sh.r, lb);
          const int64_t nvalid = std::max<int64_t>(0, std::min<int64_t>(nb, N - g * nb));
          launch_kbuild_cross(h->cfg.kernel, (const T*)h->scr.Qs.p + m0 * d, mv, mp, Xs + g * nb * d, nvalid,
                              nb, d, h->sf2, VT + lb * nb, ldv, st);
        }
      }
      {  // partial means of this batch: alpha^T (own columns) * K*^T (own columns)
        PhaseScope ps(h, &tm.mean);
        if (nloc > 0)
          launch_gemm_nt(64, (T*)h->scr.MT.p + m0, ldm, (const T*)h->YTloc.p, ldy, VT, ldv, RHS_ROWS, mp,
                         nloc, 0, 1, st);
        else
          HIPCHK(h, hipMemset2DAsync((T*)h->scr.MT.p + m0, (size_t)ldm * sizeof(T), 0, (size_t)mp * sizeof(T), RHS_ROWS, st));
      }
      if (var) {
        // Forward substitution V^T <- V^T L^-T over the block-cyclic columns with one-block
        // look-ahead, as in the factorisation: the update of block p is split into the STRIP
        // (the columns of block p+1, on the rank that owns them) and the REST; the look-ahead
        // stream then solves block p+1 on its owner and broadcasts it (into the other Sv
        // buffer) while the main stream runs the rest of update p on every rank.
        PhaseScope ps(h, &tm.trsm);
        COMMCHK(shard_fwd_sweep(h, sh, VT, ldv, mp, 0, SvB));
      }
      if (var) {
        PhaseScope ps(h, &tm.var);
        launch_var_rows(VT, ldv, mv, nloc, 0.0, (T*)h->var.p + m0, st);  // minus the local sum of squares
      }
    }
    {
      PhaseScope ps(h, &tm.mean);
      {
        PhaseScope pc(h, &tm.comm);
        COMMCHK(cm->allreduce(h, (T*)h->scr.MT.p, (size_t)RHS_ROWS * ldm, COMM_SUM));
      }
      launch_unpack_rhs((const T*)h->scr.MT.p, ldm, M, k, 1.0, (T*)h->meanout.p, st);
    }
    if (var) {
      PhaseScope ps(h, &tm.var);
      {
        PhaseScope pc(h, &tm.comm);
        COMMCHK(cm->allreduce(h, (T*)h->var.p, (size_t)M, COMM_SUM));
      }
      launch_add_scalar((T*)h->var.p, M, h->sf2, st);
    }
    if (!h->discard_out && (rc = deliver_mean_var<T>(h, mean, var, M, mem_kind))) return rc;
  }
  return finish_call(h);
}

void destroy_comm(gpx_handle* h) {
  delete h->comm;
  h->comm = nullptr;
}

}  // namespace

extern "C" {

int gpx_comm_unique_id(void* id128) try {
  if (!id128) return GPX_E_ARG;
  std::string err;
  RcclApi* api = rccl_api(&err);
  if (!api) {
    g_create_error = err;
    return GPX_E_COMM;
  }
  return api->GetUniqueId(id128) == 0 ? GPX_OK : GPX_E_COMM;
}
GPX_CATCH_ALL

int gpx_comm_init(gpx_handle* h, const void* id128) try {
  if (!h || !id128) return GPX_E_ARG;
  if (h->comm) return fail(h, GPX_E_ARG, "gpx_comm_init: communicator already initialised");
  HIPCHK(h, hipSetDevice(h->cfg.device));
  std::string err;
  RcclApi* api = rccl_api(&err);
  if (!api) return fail(h, GPX_E_COMM, err.c_str());
  RcclComm* c = new (std::nothrow) RcclComm();
  if (!c) return fail(h, GPX_E_NOMEM, "out of host memory");
  c->api = api;
  c->rank = h->cfg.rank;
  c->world = h->cfg.world;
  Id128 id;
  memcpy(id.b, id128, 128);
  const int rc = api->CommInitRank(&c->comm, c->world, id, c->rank);
  if (rc != 0) {
    h->err = std::string("ncclCommInitRank failed: ") + api->GetErrorString(rc);
    c->comm = nullptr;
    delete c;
    return GPX_E_COMM;
  }
  h->comm = c;
  return GPX_OK;
}
GPX_CATCH_ALL

int gpx_comm_init_host(gpx_handle* h, const gpx_host_comm* vt) try {
  if (!h || !vt || !vt->bcast || !vt->allgather || !vt->reduce || !vt->allreduce) return GPX_E_ARG;
  if (h->comm) return fail(h, GPX_E_ARG, "gpx_comm_init_host: communicator already initialised");
  HostComm* c = new (std::nothrow) HostComm();
  if (!c) return fail(h, GPX_E_NOMEM, "out of host memory");
  c->vt = *vt;
  c->rank = h->cfg.rank;
  c->world = h->cfg.world;
  h->comm = c;
  return GPX_OK;
}
GPX_CATCH_ALL

}  // extern "C"
