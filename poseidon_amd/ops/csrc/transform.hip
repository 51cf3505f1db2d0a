// DataTransformer on the device (reference src/caffe/data_transformer.cpp,
// which runs per datum on a host thread): raw uint8 records -> mean-subtracted,
// cropped, mirrored, scaled NCHW batch at the compute dtype, one launch per
// batch. Pure streaming: a thread produces 8 consecutive outputs of the flat
// tensor (one aligned 16-byte bf16 store, two for fp32). A group inside one
// output row fetches its 8 source bytes and 8 mean values as blocks; one that
// straddles rows, planes or images reads them one by one (a quarter of the
// traffic, L2-resident rows); a ragged tail of < 8 elements is stored scalar.
// Index walk and arithmetic: ps_transform.h. Never build this file with
// fast-math.

#include "ps_common.h"
#include "ps_transform.h"

namespace ps {

template <typename OutT>
__global__ void data_transform_k(const uint8_t* __restrict__ raw,
                                 const int* __restrict__ params,
                                 const float* __restrict__ mean,
                                 OutT* __restrict__ out, TransformGeom g,
                                 int64_t total) {
  constexpr int V = PS_TRANSFORM_VEC;
  typedef OutT vec_t __attribute__((ext_vector_type(V)));
  const int64_t ngroups = cdiv64(total, V);
  for (int64_t grp = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
       grp < ngroups; grp += (int64_t)gridDim.x * blockDim.x) {
    const int64_t flat0 = grp * V;
    const int count = total - flat0 >= V ? V : (int)(total - flat0);
    if (count == V) {
      float v[V];  // constant count: unrolled, stays in registers
      ps_transform_group(g, raw, params, mean, flat0, V, v);
      vec_t o;
#pragma unroll
      for (int j = 0; j < V; ++j) {
        OutT r;
        from_f32(v[j], r);
        o[j] = r;
      }
      *(vec_t*)&out[flat0] = o;
    } else {  // ragged tail: the last thread only
      TransformCursor p = ps_transform_decode(g, params, flat0);
      for (int j = 0; j < count; ++j) {
        if (j) ps_transform_next(g, params, p);
        from_f32(ps_transform_value(g, p, raw, mean), out[flat0 + j]);
      }
    }
  }
}

template <typename OutT>
void data_transform_launch(const uint8_t* raw, const int* params,
                           const float* mean, OutT* out,
                           const TransformGeom* g, hipStream_t s) {
  const int64_t total = (int64_t)g->N * g->C * g->Ho * g->Wo;
  if (total == 0) return;
  hipLaunchKernelGGL(data_transform_k<OutT>,
                     ew_grid(cdiv64(total, PS_TRANSFORM_VEC)), dim3(256), 0, s,
                     raw, params, mean, out, *g, total);
}

}  // namespace ps

extern "C" {
void ps_data_transform_f32(const uint8_t* raw, const int* params,
                           const float* mean, float* out,
                           const TransformGeom* g, hipStream_t s) {
  ps::data_transform_launch<float>(raw, params, mean, out, g, s);
}
void ps_data_transform_bf16(const uint8_t* raw, const int* params,
                            const float* mean, void* out,
                            const TransformGeom* g, hipStream_t s) {
  ps::data_transform_launch<__bf16>(raw, params, mean, (__bf16*)out, g, s);
}
}
