// rb_comm.hip — RCCL, resolved at run time (include/rainbow_hip.h: rb_comm_*).  Prefers the librccl the process already has (PyTorch
// ships one: the communicator then lives in the same library instance as torch.distributed's), else the ROCm installation's.
#include "rb_common.h"

#include <string.h>

#include <new>

#if !defined(RB_HOST_INTERP)
#include <dlfcn.h>
struct RbNcclUniqueId { char internal[128]; };
struct RbNccl {
  void* h;
  int (*GetUniqueId)(RbNcclUniqueId*);
  int (*CommInitRank)(void**, int, RbNcclUniqueId, int);
  int (*CommDestroy)(void*);
  int (*AllGather)(const void*, void*, size_t, int, void*, hipStream_t);
  const char* (*GetErrorString)(int);
};
static RbNccl* rb_nccl() {
  static RbNccl n;
  static int state = 0;        // 0 untried, 1 ok, -1 unavailable
  if (state == 0) {
    const char* names[] = {"librccl.so", "librccl.so.1", "/opt/rocm/lib/librccl.so", "/opt/rocm/lib/librccl.so.1"};
    n.h = nullptr;
    for (const char* nm : names) if ((n.h = dlopen(nm, RTLD_NOW | RTLD_NOLOAD | RTLD_GLOBAL))) break;     // already loaded?
    if (!n.h) for (const char* nm : names) if ((n.h = dlopen(nm, RTLD_NOW | RTLD_GLOBAL))) break;
    state = -1;
    if (n.h) {
      n.GetUniqueId = (int (*)(RbNcclUniqueId*))dlsym(n.h, "ncclGetUniqueId");
      n.CommInitRank = (int (*)(void**, int, RbNcclUniqueId, int))dlsym(n.h, "ncclCommInitRank");
      n.CommDestroy = (int (*)(void*))dlsym(n.h, "ncclCommDestroy");
      n.AllGather = (int (*)(const void*, void*, size_t, int, void*, hipStream_t))dlsym(n.h, "ncclAllGather");
      n.GetErrorString = (const char* (*)(int))dlsym(n.h, "ncclGetErrorString");
      if (n.GetUniqueId && n.CommInitRank && n.CommDestroy && n.AllGather && n.GetErrorString) state = 1;
    }
  }
  return state == 1 ? &n : nullptr;
}
#define RB_NCCL_TRY(n, expr)                                                                          \
  do {                                                                                                \
    const int r_ = (expr);                                                                            \
    if (r_ != 0) { rb_set_error("%s failed: %s", #expr, (n)->GetErrorString(r_)); return RB_ERR_HIP; } \
  } while (0)
#endif
struct rb_comm {
  void* comm;
  int world, rank;
  hipStream_t last_stream = nullptr;   // stream of the last all-gather (rb_comm_destroy waits for it)
  int used = 0;
};

extern "C" {

int rb_comm_available(void) {
#if defined(RB_HOST_INTERP)
  return 0;
#else
  return rb_nccl() ? 1 : 0;        // dlopen + dlsym only: no bootstrap id, no listener thread
#endif
}

int rb_comm_unique_id(void* id128) {
  RB_REQUIRE(id128 != nullptr, "rb_comm_unique_id: NULL argument");
#if defined(RB_HOST_INTERP)
  rb_set_error("rb_comm_unique_id: RCCL is not part of the host-interpreted test build");
  return RB_ERR_STATE;
#else
  RbNccl* n = rb_nccl();
  if (!n) { rb_set_error("rb_comm_unique_id: librccl.so could not be loaded (dlopen)"); return RB_ERR_STATE; }
  static_assert(sizeof(RbNcclUniqueId) == 128, "ncclUniqueId is 128 bytes");
  RB_NCCL_TRY(n, n->GetUniqueId(reinterpret_cast<RbNcclUniqueId*>(id128)));
  return RB_OK;
#endif
}

int rb_comm_create(rb_comm_t** out, const void* id128, int32_t world, int32_t rank) {
  RB_REQUIRE(out && id128, "rb_comm_create: NULL argument");
  RB_REQUIRE(world >= 1 && rank >= 0 && rank < world, "rb_comm_create: rank must be in [0, world)");
#if defined(RB_HOST_INTERP)
  rb_set_error("rb_comm_create: RCCL is not part of the host-interpreted test build");
  return RB_ERR_STATE;
#else
  RbNccl* n = rb_nccl();
  if (!n) { rb_set_error("rb_comm_create: librccl.so could not be loaded (dlopen)"); return RB_ERR_STATE; }
  RbNcclUniqueId id;
  memcpy(&id, id128, sizeof(id));
  void* c = nullptr;
  RB_NCCL_TRY(n, n->CommInitRank(&c, world, id, rank));
  rb_comm* rc = new (std::nothrow) rb_comm();
  if (!rc) { n->CommDestroy(c); rb_set_error("rb_comm_create: host OOM"); return RB_ERR_OOM; }
  rc->comm = c; rc->world = world; rc->rank = rank;
  *out = rc;
  return RB_OK;
#endif
}

int rb_comm_destroy(rb_comm_t* comm) {
  if (!comm) return RB_OK;
#if !defined(RB_HOST_INTERP)
  RbNccl* n = rb_nccl();
  // the all-gather of the last exchange may still be in flight on the stream it was issued on
  if (comm->used) (void)hipStreamSynchronize(comm->last_stream);
  if (n && comm->comm) n->CommDestroy(comm->comm);
#endif
  delete comm;
  return RB_OK;
}

}  // extern "C"

// (C++ linkage: what rb_learner_exchange_rccl needs of the communicator, learner_internal.h)
int rb_comm_world(const rb_comm_t* comm) { return comm->world; }
int rb_comm_all_gather_f32(rb_comm_t* comm, const float* send, float* recv, size_t count, hipStream_t stream) {
#if defined(RB_HOST_INTERP)
  (void)comm; (void)send; (void)recv; (void)count; (void)stream;
  rb_set_error("rb_learner_exchange_rccl: RCCL is not part of the host-interpreted test build");
  return RB_ERR_STATE;
#else
  RbNccl* n = rb_nccl();
  if (!n) { rb_set_error("rb_learner_exchange_rccl: librccl.so could not be loaded (dlopen)"); return RB_ERR_STATE; }
  RB_NCCL_TRY(n, n->AllGather(send, recv, count, /* ncclFloat32 */ 7, comm->comm, stream));
  comm->last_stream = stream; comm->used = 1;
  return RB_OK;
#endif
}
