// tensor_norms.h — per-tensor norms of a flat parameter-shaped buffer: for every tensor of rb_learner_param_layout, in its order,
// sum a^2, sum (a - b)^2 and max |a| — weight norms, gradient norms and the online-target distance per layer, where k_step_stats
// reports one global gradient norm.  Included by learner.hip only, after unit_recycle.h (rb_redo_block_sum: the summation order)
// and param_reset.h (reset_table: the tensors).  Never on the per-step path: two launches of their own.
//
//   k_tensor_partials   one workgroup per 4096-element chunk of ONE tensor (a tensor's chunks are cut from its own first element,
//                       so its partials do not depend on where it sits in the buffer); thread t takes the flat-aligned quads
//                       t, t + 256, ... of the chunk's range in index order — a 16-byte load where the quad lies inside the range,
//                       element by element at its edges (tensor offsets are no multiples of 4) — and sums in double; then
//                       rb_redo_block_sum's fold: the fixed butterfly inside a wave, the waves in order
//   k_tensor_fold       one workgroup per tensor: thread t adds the chunks t, t + 256, ... in index order, then the same fold
// A NaN in a or b anywhere in a tensor makes all three of that tensor's values NaN (a maximum alone would drop it).
#pragma once
#include "learner_internal.h"

#define RB_TN_CHUNK 4096
#define RB_TN_THREADS 256         // the summation order holds at exactly this many threads (rb_redo_block_sum)
#define RB_TN_PART 4              // doubles per chunk: sum a^2, sum (a - b)^2, max |a|, 1.0 if a NaN was seen

// By value in the kernels' argument blocks: read through the scalar path, the walk over it is block-uniform
struct TensorRow {
  int32_t off, count, chunk0, pad_;       // floats [off, off + count) of the flat buffer; its chunks are [chunk0, chunk0 + ceil(count / 4096))
};
struct TensorTable {
  int32_t n, chunks;
  TensorRow t[RB_RESET_MAX_DESC];
};

static void tensor_table(const Layout& L, TensorTable* T) {
  ResetTable R;
  reset_table(L, 0.0f, 0.0f, 0.0f, &R);           // alpha = 0: every tensor has its entry, in rb_learner_param_layout's order
  memset(T, 0, sizeof(*T));
  T->n = R.n;
  int chunk = 0;
  for (int k = 0; k < R.n; ++k) {
    T->t[k].off = R.d[k].off; T->t[k].count = R.d[k].count; T->t[k].chunk0 = chunk;
    chunk += (int)rb_div_up(R.d[k].count, RB_TN_CHUNK);
  }
  T->chunks = chunk;
}

// the largest of a workgroup's 256 doubles (no NaN among them): butterfly inside a wave, then the waves (all threads call)
__device__ __forceinline__ double rb_tn_block_max(double v, double* lds4) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v = fmax(v, __shfl_xor(v, m, 64));
  __syncthreads();
  if (rb_lane() == 0) lds4[rb_wave()] = v;
  __syncthreads();
  return fmax(fmax(lds4[0], lds4[1]), fmax(lds4[2], lds4[3]));
}

struct TnAcc {
  double sq, df, mx, bad;
};
__device__ __forceinline__ void rb_tn_add(TnAcc& s, float a, float b) {
  const double x = (double)a, e = x - (double)b;
  s.sq += x * x;
  s.df += e * e;
  s.mx = fmax(s.mx, fabs(x));
  if (a != a || b != b) s.bad = 1.0;
}

extern "C" {

__global__ __launch_bounds__(RB_TN_THREADS) void k_tensor_partials(TensorTable T, const float* a, const float* b, double* part) {
  __shared__ double s_w[4];
  const int c = (int)blockIdx.x;
  int k = 0;
  for (int j = 1; j < T.n; ++j)
    if (c >= T.t[j].chunk0) k = j;                                    // block-uniform
  const int lo = T.t[k].off + (c - T.t[k].chunk0) * RB_TN_CHUNK;
  const int end = T.t[k].off + T.t[k].count;
  const int hi = lo + RB_TN_CHUNK < end ? lo + RB_TN_CHUNK : end;
  TnAcc s;
  s.sq = 0.0; s.df = 0.0; s.mx = 0.0; s.bad = 0.0;
  const int q1 = (hi - 1) >> 2;
  for (int q = (lo >> 2) + (int)threadIdx.x; q <= q1; q += RB_TN_THREADS) {
    const int e0 = 4 * q;
    if (e0 >= lo && e0 + 4 <= hi) {
      const float4 x = rb_ld4(a + e0);
      const float4 y = b ? rb_ld4(b + e0) : x;
      rb_tn_add(s, x.x, y.x); rb_tn_add(s, x.y, y.y); rb_tn_add(s, x.z, y.z); rb_tn_add(s, x.w, y.w);
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (e0 + e >= lo && e0 + e < hi) {
          const float x = a[e0 + e];
          rb_tn_add(s, x, b ? b[e0 + e] : x);
        }
    }
  }
  const double sq = rb_redo_block_sum(s.sq, s_w);
  const double df = rb_redo_block_sum(s.df, s_w);
  const double mx = rb_tn_block_max(s.mx, s_w);
  const double bad = rb_tn_block_max(s.bad, s_w);
  if (threadIdx.x == 0) {
    double* o = part + (int64_t)c * RB_TN_PART;
    o[0] = sq; o[1] = df; o[2] = mx; o[3] = bad;
  }
}

__global__ __launch_bounds__(RB_TN_THREADS) void k_tensor_fold(TensorTable T, const double* part, int has_b, double* out) {
  __shared__ double s_w[4];
  const int k = (int)blockIdx.x;
  const int c0 = T.t[k].chunk0, nc = (T.t[k].count + RB_TN_CHUNK - 1) / RB_TN_CHUNK;
  double sq = 0.0, df = 0.0, mx = 0.0, bad = 0.0;
  for (int c = (int)threadIdx.x; c < nc; c += RB_TN_THREADS) {
    const double* p = part + (int64_t)(c0 + c) * RB_TN_PART;
    sq += p[0]; df += p[1]; mx = fmax(mx, p[2]); bad = fmax(bad, p[3]);
  }
  sq = rb_redo_block_sum(sq, s_w);
  df = rb_redo_block_sum(df, s_w);
  mx = rb_tn_block_max(mx, s_w);
  bad = rb_tn_block_max(bad, s_w);
  if (threadIdx.x == 0) {
    const double nan = __builtin_nan("");
    out[3 * k] = bad > 0.0 ? nan : sq;
    out[3 * k + 1] = bad > 0.0 ? nan : has_b ? df : 0.0;
    out[3 * k + 2] = bad > 0.0 ? nan : mx;
  }
}

}  // extern "C"

// The partials' scratch, [chunks][4] doubles per handle.  The handle has no room for it, so it is kept beside it: allocated by a
// handle's first rb_learner_tensor_norms, released by rb_learner_destroy.
#include <map>
#include <mutex>
static std::mutex g_tn_mutex;
static std::map<const rb_learner*, double*> g_tn_scratch;
static void tensor_norms_release(const rb_learner* l) {
  std::lock_guard<std::mutex> lock(g_tn_mutex);
  auto it = g_tn_scratch.find(l);
  if (it == g_tn_scratch.end()) return;
  rb_dev_free(it->second);
  g_tn_scratch.erase(it);
}
static int tensor_norms_scratch(const rb_learner* l, int chunks, double** out) {
  std::lock_guard<std::mutex> lock(g_tn_mutex);
  auto it = g_tn_scratch.find(l);
  if (it == g_tn_scratch.end()) {
    double* p = nullptr;
    RB_HIP_TRY(rb_dev_malloc((void**)&p, (size_t)chunks * RB_TN_PART * sizeof(double)));
    it = g_tn_scratch.emplace(l, p).first;
  }
  *out = it->second;
  return RB_OK;
}

extern "C" {

int rb_learner_tensor_norms(rb_learner_t* l, const float* a_dev, const float* b_dev, double* out_dev, rb_stream_t stream_) {
  RB_REQUIRE(l != nullptr, "rb_learner_tensor_norms: NULL handle (l)");
  RB_REQUIRE(a_dev != nullptr, "rb_learner_tensor_norms: NULL a_dev");
  RB_REQUIRE(out_dev != nullptr, "rb_learner_tensor_norms: NULL out_dev");
  RB_REQUIRE((uintptr_t)a_dev % 16 == 0, "rb_learner_tensor_norms: a_dev must be 16-byte aligned");
  RB_REQUIRE((uintptr_t)b_dev % 16 == 0, "rb_learner_tensor_norms: b_dev must be 16-byte aligned");
  RB_REQUIRE((uintptr_t)out_dev % 8 == 0, "rb_learner_tensor_norms: out_dev must be 8-byte aligned");
  RB_REQUIRE(l->L.n_params * 4 < (int64_t)0x7fffffff, "rb_learner_tensor_norms: the flat parameter buffer must be smaller than 2 GiB");
  hipStream_t stream = (hipStream_t)stream_;
  RB_FLUSH_UPDATE(l, stream);          // a pending pass moves the parameters, the target and the moments: it runs before they are read
  if (a_dev == l->grads || b_dev == l->grads) {
    if (l->dw_deferred) {
      rb_set_error("rb_learner_tensor_norms: the hidden layer's weight gradient was not materialised (RB_LEARNER_FUSE_FC_H_DW); call "
                   "rb_learner_clip_adam first");
      return RB_ERR_STATE;
    }
    RB_MATERIALIZE_SIGMA(l, stream);
  }
  TensorTable T;
  tensor_table(l->L, &T);
  double* part = nullptr;
  const int rc = tensor_norms_scratch(l, T.chunks, &part);
  if (rc != RB_OK) return rc;
  RB_LAUNCH(k_tensor_partials, dim3((unsigned)T.chunks), dim3(RB_TN_THREADS), stream, T, a_dev, b_dev, part);
  RB_LAUNCH_CHECK();
  RB_LAUNCH(k_tensor_fold, dim3((unsigned)T.n), dim3(RB_TN_THREADS), stream, T, (const double*)part, b_dev ? 1 : 0, out_dev);
  RB_LAUNCH_CHECK();
  return RB_OK;
}

}  // extern "C"
