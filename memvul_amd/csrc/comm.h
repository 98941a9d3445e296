// Part of engine.hip: the multi-GPU exchange (Comm, engine.hip) — RCCL bound directly: its entry points resolved from one table, the staging buffers grown by
// one helper, and the mv_comm_* entries.  Nothing else in the library reads this state; mv_destroy tears it down first.

namespace {

// a staging buffer of mv_comm_allgather, grown to `bytes` (what it held is not kept)
int comm_grow(mv_handle* h, void** p, int64_t* cap, int64_t bytes) {
  if (*cap >= bytes) return MV_OK;
  if (*p) hipFree(*p);
  *p = nullptr; *cap = 0;
  HIPCHK(h, hipMalloc(p, (size_t)bytes));
  *cap = bytes;
  return MV_OK;
}

}  // namespace

extern "C" {

// ---- multi-GPU exchange: RCCL bound directly ---------------------------------------------------
// librccl.so is opened at run time (never linked).  The unique id is drawn by rank 0 (mv_comm_unique_id) and handed to every
// rank's mv_comm_init as BYTES: how they travel is the host's business (memvul_amd/distributed.py broadcasts them over its
// rendezvous socket — no id file in a shared temp directory, no single-node assumption).
int mv_comm_prepare(mv_handle* h) try {
  if (!h) return MV_ERR_INVALID;
  Comm& c = h->comm;
  if (c.lib) return MV_OK;
  for (const char* name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"}) {
    c.lib = dlopen(name, RTLD_NOW | RTLD_LOCAL);
    if (c.lib) break;
  }
  if (!c.lib) return fail(h, MV_ERR_HIP, std::string("mv_comm_prepare: cannot open librccl.so: ") + dlerror());
  const struct { const char* name; void** slot; bool required; } syms[] = {
      {"ncclGetUniqueId", (void**)&c.GetUniqueId, true},   {"ncclCommInitRank", (void**)&c.CommInitRank, true},
      {"ncclAllGather", (void**)&c.AllGather, true},       {"ncclCommDestroy", (void**)&c.CommDestroy, true},
      {"ncclGetErrorString", (void**)&c.GetErrorString, true},
      {"ncclGetVersion", (void**)&c.GetVersion, false},    {"ncclCommCount", (void**)&c.CommCount, false},
      {"ncclCommUserRank", (void**)&c.CommUserRank, false},  // the optional three: mv_comm_info
  };
  for (const auto& s : syms) {
    *s.slot = dlsym(c.lib, s.name);
    if (!*s.slot && s.required) { dlclose(c.lib); c.lib = nullptr; return fail(h, MV_ERR_HIP, std::string("mv_comm_prepare: librccl.so lacks ") + s.name); }
  }
  return MV_OK;
} catch (...) { return on_exception(h); }

int mv_comm_unique_id(mv_handle* h, void* id_out, int capacity) try {
  if (!h || !id_out) return MV_ERR_INVALID;
  if (capacity < (int)sizeof(ncclUniqueId)) return fail(h, MV_ERR_INVALID, "mv_comm_unique_id: buffer smaller than ncclUniqueId (128 bytes)");
  if (int rc = mv_comm_prepare(h)) return rc;
  HIPCHK(h, hipSetDevice(h->device));
  ncclUniqueId id;
  ncclResult_t r = h->comm.GetUniqueId(&id);
  if (r != ncclSuccess) return fail(h, MV_ERR_HIP, std::string("ncclGetUniqueId: ") + h->comm.GetErrorString(r));
  std::memcpy(id_out, &id, sizeof(id));
  return (int)sizeof(id);
} catch (...) { return on_exception(h); }

int mv_comm_init(mv_handle* h, int rank, int world, const void* id, int id_bytes) try {
  if (!h || world < 1 || rank < 0 || rank >= world) return fail(h, MV_ERR_INVALID, "mv_comm_init: bad rank / world");
  Comm& c = h->comm;
  if (c.comm) return fail(h, MV_ERR_STATE, "mv_comm_init: communicator already initialised");
  // rank / world are recorded only once the init has SUCCEEDED: a failed init leaves the handle in its one-rank state (the
  // gather is then a copy) instead of a world without a communicator
  if (world == 1 && !id) { c.rank = 0; c.world = 1; return MV_OK; }  // no transport needed (with an id: a real 1-rank communicator, the GPU-box test)
  if (!id || id_bytes != (int)sizeof(ncclUniqueId)) return fail(h, MV_ERR_INVALID, "mv_comm_init: the 128-byte unique id of rank 0 (mv_comm_unique_id) is required");
  if (int rc = mv_comm_prepare(h)) return rc;
  HIPCHK(h, hipSetDevice(h->device));
  ncclUniqueId uid;
  std::memcpy(&uid, id, sizeof(uid));
  ncclResult_t r = c.CommInitRank(&c.comm, world, uid, rank);
  if (r != ncclSuccess) { c.comm = nullptr; return fail(h, MV_ERR_HIP, std::string("ncclCommInitRank: ") + c.GetErrorString(r)); }
  c.rank = rank;
  c.world = world;
  return MV_OK;
} catch (...) { return on_exception(h); }

// What the transport IS, as RCCL itself reports it: info[0] = ranks of the live communicator by ncclCommCount (0: no
// communicator — one rank, or the run is on another transport), info[1] = this rank in it by ncclCommUserRank, info[2] = the
// RCCL version code of ncclGetVersion (0 while librccl.so is not open), info[3] = the world mv_comm_allgather will gather over.
int mv_comm_info(mv_handle* h, int* info, int n) try {
  if (!h || !info || n < 4) return fail(h, MV_ERR_INVALID, "mv_comm_info: int[4] required");
  const Comm& c = h->comm;
  info[0] = info[1] = info[2] = 0;
  info[3] = c.world;
  if (c.lib && c.GetVersion) { int v = 0; if (c.GetVersion(&v) == ncclSuccess) info[2] = v; }
  if (c.comm) {
    int n_ranks = -1, r = -1;
    if (c.CommCount && c.CommCount(c.comm, &n_ranks) == ncclSuccess) info[0] = n_ranks;
    if (c.CommUserRank && c.CommUserRank(c.comm, &r) == ncclSuccess) info[1] = r;
  }
  return MV_OK;
} catch (...) { return on_exception(h); }

int mv_comm_allgather(mv_handle* h, const void* send, void* recv, int64_t bytes_per_rank) try {
  if (!h || !send || !recv || bytes_per_rank <= 0) return fail(h, MV_ERR_INVALID, "mv_comm_allgather: bad argument");
  Comm& c = h->comm;
  if (c.world == 1 && !c.comm) { std::memcpy(recv, send, (size_t)bytes_per_rank); return MV_OK; }
  if (!c.comm) return fail(h, MV_ERR_STATE, "mv_comm_allgather: mv_comm_init first");
  HIPCHK(h, hipSetDevice(h->device));
  if (int rc = sync_all(h)) return rc;
  hipStream_t st = h->work[0].stream;
  const int64_t total = bytes_per_rank * c.world;
  if (int rc = comm_grow(h, &c.send, &c.send_cap, bytes_per_rank)) return rc;
  if (int rc = comm_grow(h, &c.recv, &c.recv_cap, total)) return rc;
  HIPCHK(h, hipMemcpyAsync(c.send, send, (size_t)bytes_per_rank, hipMemcpyHostToDevice, st));
  ncclResult_t r = c.AllGather(c.send, c.recv, (size_t)bytes_per_rank, ncclChar, c.comm, st);
  if (r != ncclSuccess) return fail(h, MV_ERR_HIP, std::string("ncclAllGather: ") + c.GetErrorString(r));
  HIPCHK(h, hipMemcpyAsync(recv, c.recv, (size_t)total, hipMemcpyDeviceToHost, st));
  HIPCHK(h, hipStreamSynchronize(st));
  return MV_OK;
} catch (...) { return on_exception(h); }

int mv_comm_destroy(mv_handle* h) try {
  if (!h) return MV_ERR_INVALID;
  Comm& c = h->comm;
  (void)hipSetDevice(h->device);
  if (c.comm) { c.CommDestroy(c.comm); c.comm = nullptr; }
  if (c.send) { hipFree(c.send); c.send = nullptr; c.send_cap = 0; }
  if (c.recv) { hipFree(c.recv); c.recv = nullptr; c.recv_cap = 0; }
  c.world = 1; c.rank = 0;
  return MV_OK;
} catch (...) { return on_exception(h); }

}  // extern "C"
