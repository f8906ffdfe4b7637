// Fused Adam step (FairSeq `adam` semantics: decoupled weight decay applied as p -= wd*lr*p, bias-corrected
// step size lr*sqrt(1-b2^t)/(1-b1^t), denominator sqrt(v)+eps) over one parameter tensor: reads the fp32
// gradient accumulated by the backward kernels, updates fp32 moments and the fp32 master copy, and writes
// the working-precision parameter — one HBM pass (28-30 B per element) instead of ~10 eager elementwise ops.
// Launch flags of the reference: --optimizer adam --adam-betas '(0.9, 0.999)' --adam-eps 1e-8
// --weight-decay 0.01 (mDT/experiments/hateful_discussions/run_train.sh:38).
#include "common.hpp"

namespace mdt {

// The guard state the norm finaliser writes and the guarded kernels read (include/mdt_hip.h: mdt_adam_guard).
// GUARD = false is the plain step: `grad_scale` is the optional device scalar, the host's step size is used as given.
// GUARD = true reads the effective scale from the guard state, stores NOTHING when the update is skipped, and takes the
// step size of the updates actually applied once any update has been skipped (until then the host's count is the
// applied count, and the arithmetic is the plain step's bit for bit).
template <bool GUARD>
__device__ __forceinline__ bool adam_scale_and_step(const float* __restrict__ grad_scale, const mdt_adam_guard* __restrict__ guard,
                                                    float& gs, float& step_size) {
  if constexpr (GUARD) {
    if (guard->skip) return false;
    gs = guard->scale;
    if (guard->skipped) step_size = guard->step_size;
  } else {
    gs = grad_scale ? grad_scale[0] : 1.0f;
  }
  return true;
}

// The weight average of the `_ema` entry points (FairSeq --store-ema).  EMA = false: an empty argument, the plain kernels —
// the same instantiations as before the average existed.  EMA = true: after p is final, e = d * e + (1.0f - d) * p on the fp32
// average, p being the value stored to the master (to the parameter where there is none); d == 0 stores p itself, so the
// copy is exact for every p.  A skipped update returns before anything is read: the average keeps its bits too.
template <bool EMA> struct EmaOne {};
template <> struct EmaOne<true> { float* ema; float decay; };
template <bool EMA> struct EmaTable {};
template <> struct EmaTable<true> { float* const* ema; float decay; };     // one pointer per table entry, NULL: no average

__device__ __forceinline__ void ema_update(float* __restrict__ ema, int64_t i, float d, float p) {
  const float e = d * ema[i] + (1.0f - d) * p;
  ema[i] = d == 0.0f ? p : e;
}

// Parameter groups of the `_group(s)` entry points (include/mdt_hip.h: mdt_adam_group).  GROUPS = false: an empty argument, the
// kernels without groups.  GROUPS = true: the tensor's record replaces the launch's hyper-parameters, once per tensor (per chunk
// in the table form): lr_t = lr * lr_scale and step_size_t = step_size * lr_scale, one fp32 product each, the second AFTER
// adam_scale_and_step so that the guard's own step size is scaled as well; wd_t = weight_decay of the record.
template <bool GROUPS> struct GroupOne {};
template <> struct GroupOne<true> { mdt_adam_group g; };
template <bool GROUPS> struct GroupTable {};
template <> struct GroupTable<true> { const mdt_adam_group* groups; };      // one record per table entry, by TENSOR

__device__ __forceinline__ void group_hyper(const mdt_adam_group g, float& lr, float& wd, float& step_size) {
  lr = lr * g.lr_scale;
  step_size = step_size * g.lr_scale;
  wd = g.weight_decay;
}

// The Adam update of element i, the one copy both kernels run: loads, arithmetic and stores.  → the fp32 value the weight
// average follows: what went to the master, or where there is none the parameter as stored.
template <typename T>
__device__ __forceinline__ float adam_element(int64_t i, const float* grad, float* m, float* v, float* master, T* param, float lr,
                                              float beta1, float beta2, float eps, float wd, float gs, float step_size) {
  const float g = grad[i] * gs;
  const float mi = beta1 * m[i] + (1.0f - beta1) * g;
  const float vi = beta2 * v[i] + (1.0f - beta2) * g * g;
  float p = master ? master[i] : to_f32(param[i]);
  p -= wd * lr * p;
  p -= step_size * mi / (sqrtf(vi) + eps);
  m[i] = mi;
  v[i] = vi;
  if (master) master[i] = p;
  const T stored = from_f32<T>(p);
  param[i] = stored;
  return master ? p : to_f32(stored);
}

template <typename T, bool GUARD, bool EMA, bool GROUPS>
__global__ __launch_bounds__(256) void adam_kernel(int64_t n, T* __restrict__ param, float* __restrict__ master,
                                                   const float* __restrict__ grad, float* __restrict__ m,
                                                   float* __restrict__ v, float lr, float beta1, float beta2, float eps,
                                                   float wd, float step_size, const float* __restrict__ grad_scale,
                                                   const mdt_adam_guard* __restrict__ guard, EmaOne<EMA> ea, GroupOne<GROUPS> ga) {
  float gs;
  if (!adam_scale_and_step<GUARD>(grad_scale, guard, gs, step_size)) return;
  if constexpr (GROUPS) group_hyper(ga.g, lr, wd, step_size);
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const float p = adam_element(i, grad, m, v, master, param, lr, beta1, beta2, eps, wd, gs, step_size);
    if constexpr (EMA) ema_update(ea.ema, i, ea.decay, p);
  }
}

// Tensor of chunk `chunk` in a table whose tensor t starts at chunk chunk_first[t] (monotone, chunk_first[n] = total).
__device__ __forceinline__ int tensor_of_chunk(const int64_t* __restrict__ chunk_first, int n_tensors, int64_t chunk) {
  int lo = 0, hi = n_tensors - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (chunk_first[mid] <= chunk) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// Where chunk `chunk` of such a table lies: its tensor, and the element of that tensor the chunk starts at.  base() reads
// chunk_first where the kernel asks for it: each kernel keeps the order of its loads.
struct ChunkAt {
  int tensor;
  const int64_t* first;
  int64_t chunk;
  __device__ __forceinline__ int64_t base() const { return (chunk - first[tensor]) * 4096; }
};
__device__ __forceinline__ ChunkAt chunk_at(const int64_t* __restrict__ chunk_first, int n_tensors, int64_t chunk) {
  return {tensor_of_chunk(chunk_first, n_tensors, chunk), chunk_first, chunk};
}

// Multi-tensor form: one launch walks a device table of tensors (the ~400 parameter tensors of mDT would otherwise
// cost ~400 launches of 10-20 us each).  Block b works on chunk b of 4096 elements; `chunk_first[t]` is the first
// chunk of tensor t (monotone, chunk_first[n] = total), found by binary search.
template <typename T, bool GUARD, bool EMA, bool GROUPS>
__global__ __launch_bounds__(256) void adam_multi_kernel(int n_tensors, const mdt_adam_tensor* __restrict__ tab,
                                                         const int64_t* __restrict__ chunk_first, float lr, float beta1,
                                                         float beta2, float eps, float wd, float step_size,
                                                         const float* __restrict__ grad_scale,
                                                         const mdt_adam_guard* __restrict__ guard, EmaTable<EMA> ea,
                                                         GroupTable<GROUPS> ga) {
  float gs;
  if (!adam_scale_and_step<GUARD>(grad_scale, guard, gs, step_size)) return;
  const int64_t total = chunk_first[n_tensors];
  for (int64_t chunk = blockIdx.x; chunk < total; chunk += gridDim.x) {
    const ChunkAt at = chunk_at(chunk_first, n_tensors, chunk);
    const mdt_adam_tensor t = tab[at.tensor];
    const int64_t base = at.base();
    float* ema = nullptr;
    if constexpr (EMA) ema = ea.ema[at.tensor];
    float lr_t = lr, wd_t = wd, step_size_t = step_size;
    if constexpr (GROUPS) group_hyper(ga.groups[at.tensor], lr_t, wd_t, step_size_t);
#pragma unroll 4
    for (int k = 0; k < 16; ++k) {
      const int64_t i = base + k * 256 + threadIdx.x;
      if (i >= t.numel) break;
      const float p = adam_element(i, t.grad, t.m, t.v, t.master, (T*)t.param, lr_t, beta1, beta2, eps, wd_t, gs, step_size_t);
      if constexpr (EMA) {
        if (ema) ema_update(ema, i, ea.decay, p);
      }
    }
  }
}

// The swap of mdt_ema_swap_multi: one block per 4096-element chunk of the same table.  A tensor with a master: param = T(ema)
// (restore: T(master)) — the master is the keeper of the raw weights, nothing else is written.  An fp32 tensor without one:
// param and ema trade contents (restore trades them back).  Thread t owns the 16-byte group (k * 256 + t) of the chunk's
// parameter elements: one vector load / store each where param and the fp32 source start on 16-byte boundaries and the group
// lies inside the tensor, element by element, same ownership and order, elsewhere.
template <typename T>
__global__ __launch_bounds__(256) void ema_swap_multi_kernel(int n_tensors, const mdt_adam_tensor* __restrict__ tab,
                                                             float* const* __restrict__ ema_tab,
                                                             const int64_t* __restrict__ chunk_first, int restore) {
  constexpr int N = Vec<T>::N;
  const int64_t total = chunk_first[n_tensors];
  for (int64_t chunk = blockIdx.x; chunk < total; chunk += gridDim.x) {
    const ChunkAt at = chunk_at(chunk_first, n_tensors, chunk);
    float* ema = ema_tab[at.tensor];
    if (!ema) continue;
    const mdt_adam_tensor t = tab[at.tensor];
    const int64_t base = at.base();
    T* param = (T*)t.param + base;
    const int64_t left = t.numel - base;
    if (t.master) {
      const float* src = (restore ? t.master : ema) + base;
      const bool vec = (((uintptr_t)param | (uintptr_t)src) & 15) == 0;
      for (int j = threadIdx.x * N; j < 4096; j += 256 * N) {
        if (j >= left) break;
        if (vec && j + N <= left) {
          Vec<T> o;
#pragma unroll
          for (int q = 0; q < N; q += 4) {
            const f32x4 x = *(const f32x4*)(src + j + q);
            o.set(q, x[0]); o.set(q + 1, x[1]); o.set(q + 2, x[2]); o.set(q + 3, x[3]);
          }
          *(Vec<T>*)(param + j) = o;
        } else {
          for (int q = 0; q < N && j + q < left; ++q) param[j + q] = from_f32<T>(src[j + q]);
        }
      }
    } else if constexpr (std::is_same<T, float>::value) {
      float* e = ema + base;
      const bool vec = (((uintptr_t)param | (uintptr_t)e) & 15) == 0;
      for (int j = threadIdx.x * 4; j < 4096; j += 1024) {
        if (j >= left) break;
        if (vec && j + 4 <= left) {
          const f32x4 a = *(const f32x4*)(param + j), b = *(const f32x4*)(e + j);
          *(f32x4*)(param + j) = b;
          *(f32x4*)(e + j) = a;
        } else {
          for (int q = 0; q < 4 && j + q < left; ++q) {
            const float a = param[j + q], b = e[j + q];
            param[j + q] = b;
            e[j + q] = a;
          }
        }
      }
    }
  }
}

// ---------------------------------------------------------------- global gradient norm (--clip-norm, gnorm, non-finite guard)
// Sum of squares of one 4096-element chunk, the same bits whatever the grid: thread t owns the four float4 groups
// (k * 256 + t) of the chunk and adds its 16 squares in index order, the wave sums its 64 lanes with the DPP tree
// LayerNorm uses, wave 0's lane 0 adds the four wave totals as (w0 + w1) + (w2 + w3).  No atomics; elements past the
// end of the tensor count as +0.  The groups are loaded 16 bytes at a time where the chunk starts on a 16-byte
// boundary (arena slots do) and element by element, same ownership and order, where a view starts elsewhere.
__device__ __forceinline__ float chunk_sumsq(const float* __restrict__ g, int64_t left, float* red) {
  const int tid = threadIdx.x;
  const bool vec = ((uintptr_t)g & 15) == 0;
  float acc = 0.0f;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int64_t i = (int64_t)(k * 256 + tid) * 4;
    float x0 = 0.0f, x1 = 0.0f, x2 = 0.0f, x3 = 0.0f;
    if (vec && i + 3 < left) {
      const f32x4 q = *(const f32x4*)(g + i);
      x0 = q[0]; x1 = q[1]; x2 = q[2]; x3 = q[3];
    } else {
      if (i < left) x0 = g[i];
      if (i + 1 < left) x1 = g[i + 1];
      if (i + 2 < left) x2 = g[i + 2];
      if (i + 3 < left) x3 = g[i + 3];
    }
    acc += x0 * x0;
    acc += x1 * x1;
    acc += x2 * x2;
    acc += x3 * x3;
  }
  acc = wave_sum_dpp(acc);
  if ((tid & 63) == 0) red[tid >> 6] = acc;
  __syncthreads();
  const float total = (red[0] + red[1]) + (red[2] + red[3]);
  __syncthreads();          // `red` is written again by the block's next chunk
  return total;
}

__global__ __launch_bounds__(256) void grad_sumsq_multi_kernel(int n_tensors, const mdt_adam_tensor* __restrict__ tab,
                                                               const int64_t* __restrict__ chunk_first,
                                                               float* __restrict__ partials) {
  __shared__ float red[4];
  const int64_t total = chunk_first[n_tensors];
  for (int64_t chunk = blockIdx.x; chunk < total; chunk += gridDim.x) {
    const ChunkAt at = chunk_at(chunk_first, n_tensors, chunk);
    const int64_t base = at.base();
    const float s = chunk_sumsq(tab[at.tensor].grad + base, tab[at.tensor].numel - base, red);
    if (threadIdx.x == 0) partials[chunk] = s;
  }
}

__global__ __launch_bounds__(256) void grad_sumsq_kernel(int64_t n, const float* __restrict__ grad, float* __restrict__ partials) {
  __shared__ float red[4];
  const int64_t total = (n + 4095) / 4096;
  for (int64_t chunk = blockIdx.x; chunk < total; chunk += gridDim.x) {
    const float s = chunk_sumsq(grad + chunk * 4096, n - chunk * 4096, red);
    if (threadIdx.x == 0) partials[chunk] = s;
  }
}

// One block: thread t adds partials t, t + 256, ... in index order in fp64, the 256 sums are folded by a fixed
// halving tree, thread 0 derives the guard state (FairSeq's order: the norm of the gradient AFTER multiply_grads,
// then clip_grad_norm_'s coefficient).  `reset`: the running counters start from zero at this call, whatever the
// buffer held (nothing of the guard state is read before it is written).
__global__ __launch_bounds__(256) void grad_norm_finalize_kernel(const float* __restrict__ partials, int64_t n_partials,
                                                                 float max_norm, const float* __restrict__ grad_scale,
                                                                 float lr, float beta1, float beta2, int step, int reset,
                                                                 mdt_adam_guard* __restrict__ guard) {
  __shared__ double red[256];
  const int tid = threadIdx.x;
  double acc = 0.0;
  for (int64_t i = tid; i < n_partials; i += 256) acc += (double)partials[i];
  red[tid] = acc;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) red[tid] += red[tid + o];
    __syncthreads();
  }
  if (tid != 0) return;
  const float s_in = grad_scale ? grad_scale[0] : 1.0f;
  const float gnorm = (float)((double)s_in * sqrt(red[0]));
  const bool finite = isfinite(gnorm);
  const bool clip = finite && max_norm > 0.0f && gnorm > max_norm;
  int clipped = reset ? 0 : guard->clipped, skipped = reset ? 0 : guard->skipped;
  float scale = s_in;                                   // max_norm <= 0 or no clipping: the incoming scale, bit for bit
  if (clip) scale = (float)((double)s_in * ((double)max_norm / ((double)gnorm + 1e-6)));
  skipped += finite ? 0 : 1;
  clipped += clip ? 1 : 0;
  const int applied = step - skipped;
  float step_size = 0.0f;
  if (skipped > 0 && applied > 0)
    step_size = (float)((double)lr * sqrt(1.0 - pow((double)beta2, (double)applied)) / (1.0 - pow((double)beta1, (double)applied)));
  guard->scale = scale;
  guard->gnorm = gnorm;
  guard->step_size = step_size;
  guard->skip = finite ? 0 : 1;
  guard->applied = applied;
  guard->clipped = clipped;
  guard->skipped = skipped;
  guard->reserved = 0;
}

}  // namespace mdt

using namespace mdt;

// Grid of the chunk kernels: a block per 4096-element chunk, at most 65536 blocks (each then strides over the chunks).
static unsigned chunk_grid(int64_t total_chunks) { return (unsigned)(total_chunks > 65536 ? 65536 : total_chunks); }

static float adam_step_size(float lr, float beta1, float beta2, int step) {
  const double bc1 = 1.0 - pow((double)beta1, step), bc2 = 1.0 - pow((double)beta2, step);
  return (float)(lr * sqrt(bc2) / bc1);
}

template <bool GUARD, bool EMA = false, bool GROUPS = false>
static int adam_step_multi(const char* what, void* stream, int dtype, int n_tensors, const mdt_adam_tensor* table_dev,
                           const int64_t* chunk_first_dev, int64_t total_chunks, float lr, float beta1, float beta2, float eps,
                           float weight_decay, int step, const float* grad_scale, const mdt_adam_guard* guard,
                           EmaTable<EMA> ea = {}, GroupTable<GROUPS> ga = {}) {
  if (n_tensors == 0 || total_chunks == 0) return MDT_OK;
  MDT_CHECK_ARG(table_dev && chunk_first_dev && step >= 1 && (!GUARD || guard), "%s: bad arguments", what);
  if constexpr (EMA) MDT_CHECK_ARG(ea.ema && ea.decay >= 0.0f && ea.decay <= 1.0f, "%s: ema_dev is NULL or ema_decay is outside [0, 1]", what);
  const float step_size = adam_step_size(lr, beta1, beta2, step);
  hipStream_t st = (hipStream_t)stream;
  return with_dtype(dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    return launch_plain<adam_multi_kernel<T, GUARD, EMA, GROUPS>>(what, chunk_grid(total_chunks), 256, st, n_tensors, table_dev, chunk_first_dev, lr, beta1, beta2, eps,
                                                                  weight_decay, step_size, grad_scale, guard, ea, ga);
  });
}

template <bool GUARD, bool EMA = false, bool GROUPS = false>
static int adam_step_one(const char* what, void* stream, int dtype, int64_t n, void* param, float* master, const float* grad,
                         float* m, float* v, float lr, float beta1, float beta2, float eps, float weight_decay, int step,
                         const float* grad_scale, const mdt_adam_guard* guard, EmaOne<EMA> ea = {}, GroupOne<GROUPS> ga = {}) {
  if (n == 0) return MDT_OK;
  MDT_CHECK_ARG(param && grad && m && v && step >= 1 && (!GUARD || guard), "%s: bad arguments", what);
  if constexpr (EMA) MDT_CHECK_ARG(ea.ema && ea.decay >= 0.0f && ea.decay <= 1.0f, "%s: ema is NULL or ema_decay is outside [0, 1]", what);
  const float step_size = adam_step_size(lr, beta1, beta2, step);
  const unsigned grid = (unsigned)((n + 255) / 256 > 8192 ? 8192 : (n + 255) / 256);
  hipStream_t st = (hipStream_t)stream;
  return with_dtype(dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    return launch_plain<adam_kernel<T, GUARD, EMA, GROUPS>>(what, grid, 256, st, n, (T*)param, master, grad, m, v, lr, beta1, beta2, eps, weight_decay,
                                                            step_size, grad_scale, guard, ea, ga);
  });
}

extern "C" int mdt_adam_step_multi(void* stream, int dtype, int n_tensors, const mdt_adam_tensor* table_dev,
                                   const int64_t* chunk_first_dev, int64_t total_chunks, float lr, float beta1, float beta2,
                                   float eps, float weight_decay, int step, const float* grad_scale) {
  return adam_step_multi<false>("adam_step_multi", stream, dtype, n_tensors, table_dev, chunk_first_dev, total_chunks, lr, beta1,
                                beta2, eps, weight_decay, step, grad_scale, nullptr);
}

extern "C" int mdt_adam_step(void* stream, int dtype, int64_t n, void* param, float* master, const float* grad, float* m,
                             float* v, float lr, float beta1, float beta2, float eps, float weight_decay, int step,
                             const float* grad_scale) {
  return adam_step_one<false>("adam_step", stream, dtype, n, param, master, grad, m, v, lr, beta1, beta2, eps, weight_decay, step,
                              grad_scale, nullptr);
}

extern "C" int mdt_adam_step_multi_guarded(void* stream, int dtype, int n_tensors, const mdt_adam_tensor* table_dev,
                                           const int64_t* chunk_first_dev, int64_t total_chunks, float lr, float beta1,
                                           float beta2, float eps, float weight_decay, int step, const mdt_adam_guard* guard) {
  return adam_step_multi<true>("adam_step_multi_guarded", stream, dtype, n_tensors, table_dev, chunk_first_dev, total_chunks, lr,
                               beta1, beta2, eps, weight_decay, step, nullptr, guard);
}

extern "C" int mdt_adam_step_guarded(void* stream, int dtype, int64_t n, void* param, float* master, const float* grad, float* m,
                                     float* v, float lr, float beta1, float beta2, float eps, float weight_decay, int step,
                                     const mdt_adam_guard* guard) {
  return adam_step_one<true>("adam_step_guarded", stream, dtype, n, param, master, grad, m, v, lr, beta1, beta2, eps, weight_decay,
                             step, nullptr, guard);
}

// The `_ema` forms: the same launches with the weight average riding on them (include/mdt_hip.h).
extern "C" int mdt_adam_step_multi_ema(void* stream, int dtype, int n_tensors, const mdt_adam_tensor* table_dev,
                                       const int64_t* chunk_first_dev, int64_t total_chunks, float lr, float beta1, float beta2,
                                       float eps, float weight_decay, int step, const float* grad_scale, float* const* ema_dev,
                                       float ema_decay) {
  return adam_step_multi<false, true>("adam_step_multi_ema", stream, dtype, n_tensors, table_dev, chunk_first_dev, total_chunks, lr,
                                      beta1, beta2, eps, weight_decay, step, grad_scale, nullptr, {ema_dev, ema_decay});
}

extern "C" int mdt_adam_step_ema(void* stream, int dtype, int64_t n, void* param, float* master, const float* grad, float* m,
                                 float* v, float lr, float beta1, float beta2, float eps, float weight_decay, int step,
                                 const float* grad_scale, float* ema, float ema_decay) {
  return adam_step_one<false, true>("adam_step_ema", stream, dtype, n, param, master, grad, m, v, lr, beta1, beta2, eps, weight_decay,
                                    step, grad_scale, nullptr, {ema, ema_decay});
}

extern "C" int mdt_adam_step_multi_ema_guarded(void* stream, int dtype, int n_tensors, const mdt_adam_tensor* table_dev,
                                               const int64_t* chunk_first_dev, int64_t total_chunks, float lr, float beta1,
                                               float beta2, float eps, float weight_decay, int step, const mdt_adam_guard* guard,
                                               float* const* ema_dev, float ema_decay) {
  return adam_step_multi<true, true>("adam_step_multi_ema_guarded", stream, dtype, n_tensors, table_dev, chunk_first_dev, total_chunks,
                                     lr, beta1, beta2, eps, weight_decay, step, nullptr, guard, {ema_dev, ema_decay});
}

extern "C" int mdt_adam_step_ema_guarded(void* stream, int dtype, int64_t n, void* param, float* master, const float* grad,
                                         float* m, float* v, float lr, float beta1, float beta2, float eps, float weight_decay,
                                         int step, const mdt_adam_guard* guard, float* ema, float ema_decay) {
  return adam_step_one<true, true>("adam_step_ema_guarded", stream, dtype, n, param, master, grad, m, v, lr, beta1, beta2, eps,
                                   weight_decay, step, nullptr, guard, {ema, ema_decay});
}

// The group forms (include/mdt_hip.h): per-tensor lr scale and weight decay; the guard and the average are nullable arguments.
extern "C" int mdt_adam_step_multi_groups(void* stream, int dtype, int n_tensors, const mdt_adam_tensor* table_dev,
                                          const int64_t* chunk_first_dev, int64_t total_chunks, float lr, float beta1, float beta2,
                                          float eps, int step, const mdt_adam_group* groups_dev, const float* grad_scale,
                                          const mdt_adam_guard* guard, float* const* ema_dev, float ema_decay) {
  const char* what = "adam_step_multi_groups";
  MDT_CHECK_ARG(!(grad_scale && guard), "%s: grad_scale and guard are both given (the guard state carries the scale)", what);
  MDT_CHECK_ARG(groups_dev, "%s: groups_dev is NULL (mdt_adam_step_multi* are the forms without groups)", what);
  const GroupTable<true> ga{groups_dev};
  const EmaTable<true> ea{ema_dev, ema_decay};
#define MDT_ADAM_GROUPS(G, E, ...) \
  adam_step_multi<G, E, true>(what, stream, dtype, n_tensors, table_dev, chunk_first_dev, total_chunks, lr, beta1, beta2, eps, 0.0f, step, \
                              grad_scale, guard, __VA_ARGS__, ga)
  if (guard) return ema_dev ? MDT_ADAM_GROUPS(true, true, ea) : MDT_ADAM_GROUPS(true, false, EmaTable<false>{});
  return ema_dev ? MDT_ADAM_GROUPS(false, true, ea) : MDT_ADAM_GROUPS(false, false, EmaTable<false>{});
#undef MDT_ADAM_GROUPS
}

extern "C" int mdt_adam_step_group(void* stream, int dtype, int64_t n, void* param, float* master, const float* grad, float* m,
                                   float* v, float lr, float beta1, float beta2, float eps, int step, float lr_scale,
                                   float weight_decay, const float* grad_scale, const mdt_adam_guard* guard, float* ema,
                                   float ema_decay) {
  const char* what = "adam_step_group";
  MDT_CHECK_ARG(!(grad_scale && guard), "%s: grad_scale and guard are both given (the guard state carries the scale)", what);
  MDT_CHECK_ARG(std::isfinite(lr_scale) && lr_scale >= 0.0f && std::isfinite(weight_decay) && weight_decay >= 0.0f,
                "%s: lr_scale %g and weight_decay %g must be finite and >= 0", what, (double)lr_scale, (double)weight_decay);
  const GroupOne<true> ga{{lr_scale, weight_decay}};
  const EmaOne<true> ea{ema, ema_decay};
#define MDT_ADAM_GROUP(G, E, ...) \
  adam_step_one<G, E, true>(what, stream, dtype, n, param, master, grad, m, v, lr, beta1, beta2, eps, 0.0f, step, grad_scale, guard, \
                            __VA_ARGS__, ga)
  if (guard) return ema ? MDT_ADAM_GROUP(true, true, ea) : MDT_ADAM_GROUP(true, false, EmaOne<false>{});
  return ema ? MDT_ADAM_GROUP(false, true, ea) : MDT_ADAM_GROUP(false, false, EmaOne<false>{});
#undef MDT_ADAM_GROUP
}

extern "C" int mdt_ema_swap_multi(void* stream, int dtype, int n_tensors, const mdt_adam_tensor* table_dev, float* const* ema_dev,
                                  const int64_t* chunk_first_dev, int64_t total_chunks, int restore) {
  if (n_tensors == 0 || total_chunks == 0) return MDT_OK;
  MDT_CHECK_ARG(table_dev && ema_dev && chunk_first_dev && (restore == 0 || restore == 1), "ema_swap_multi: bad arguments");
  return with_dtype(dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    return launch_plain<ema_swap_multi_kernel<T>>("ema_swap_multi", chunk_grid(total_chunks), 256, (hipStream_t)stream, n_tensors, table_dev, ema_dev,
                                                  chunk_first_dev, restore);
  });
}

extern "C" int mdt_grad_sumsq_multi(void* stream, int n_tensors, const mdt_adam_tensor* table_dev, const int64_t* chunk_first_dev,
                                    int64_t total_chunks, float* partials) {
  if (n_tensors == 0 || total_chunks == 0) return MDT_OK;
  MDT_CHECK_ARG(table_dev && chunk_first_dev && partials, "grad_sumsq_multi: bad arguments");
  return launch_plain<grad_sumsq_multi_kernel>("grad_sumsq_multi", chunk_grid(total_chunks), 256, (hipStream_t)stream, n_tensors, table_dev,
                                               chunk_first_dev, partials);
}

extern "C" int mdt_grad_sumsq(void* stream, int64_t n, const float* grad, float* partials) {
  if (n == 0) return MDT_OK;
  MDT_CHECK_ARG(n > 0 && grad && partials, "grad_sumsq: bad arguments");
  return launch_plain<grad_sumsq_kernel>("grad_sumsq", chunk_grid((n + 4095) / 4096), 256, (hipStream_t)stream, n, grad, partials);
}

extern "C" int mdt_grad_norm_finalize(void* stream, const float* partials, int64_t n_partials, float max_norm,
                                      const float* grad_scale, float lr, float beta1, float beta2, int step, int reset,
                                      mdt_adam_guard* guard) {
  MDT_CHECK_ARG(guard && n_partials >= 0 && (partials || n_partials == 0) && step >= 1, "grad_norm_finalize: bad arguments");
  hipLaunchKernelGGL(grad_norm_finalize_kernel, 1, 256, 0, (hipStream_t)stream, partials, n_partials, max_norm, grad_scale, lr,
                     beta1, beta2, step, reset, guard);
  return check_launch("grad_norm_finalize");
}
