// Device-resident keypoint records (include/rtpe_hip_records.h): the fixed-size record of every image of a batch,
// [image_id, n_people, scores[P], kpts[P][J][4]], written behind adjust + refine from the rows as they lie in device
// memory - what engine.pack_records builds on the host from the per-image lists, and transforms.get_final_preds'
// float64 affine on the way.  One workgroup per image; every float of a record is written, the zeros included.
#include "rtpe_common.h"

namespace rtpe {
namespace {

constexpr int kRecThreads = 256;

struct RecArgs {
  const float* rows;
  const float* scores;
  const int32_t* counts;
  const int32_t* image_ids;
  const double* xform;
  float* rec;
  size_t floats;          // of one record
  int C, J, cap, max_people;
};

// float i of the header [image_id, n, scores[max_people]] of an image with n people whose rows start at o
__device__ __forceinline__ float rec_header(const RecArgs& a, int image, int n, long long o, int i) {
  if (i == 0) return (float)a.image_ids[image];
  if (i == 1) return (float)n;
  return i - 2 < n ? a.scores[o + (i - 2)] : 0.f;
}

// kVec4: the header is a whole number of float4 and the records are 16-byte aligned (the (17, 30) layout: header 32
// floats, stride 8288 B) - one 16-byte store per keypoint; otherwise one 4-byte store per float
template <bool kVec4>
__global__ __launch_bounds__(kRecThreads) void pack_records_kernel(RecArgs a) {
  __shared__ int part[kRecThreads];
  const int image = blockIdx.x, tid = threadIdx.x;
  // o = sum(counts[:image]): integers, any order is exact
  int s = 0;
  for (int m = tid; m < image; m += kRecThreads) s += a.counts[m];
  part[tid] = s;
  __syncthreads();
  for (int w = kRecThreads / 2; w > 0; w >>= 1) {
    if (tid < w) part[tid] += part[tid + w];
    __syncthreads();
  }
  const long long o = part[0];
  int n = a.counts[image];
  n = n < a.max_people ? n : a.max_people;
  // nothing at or beyond `cap` is read, whatever the counts say
  if (o < 0 || o >= a.cap) n = 0;
  else if (n > a.cap - o) n = (int)(a.cap - o);
  if (n < 0) n = 0;

  float* out = a.rec + (size_t)image * a.floats;
  const int head = 2 + a.max_people;
  if (kVec4) {
    for (int i = tid; i < head / 4; i += kRecThreads) {
      float4 v;
      v.x = rec_header(a, image, n, o, 4 * i);
      v.y = rec_header(a, image, n, o, 4 * i + 1);
      v.z = rec_header(a, image, n, o, 4 * i + 2);
      v.w = rec_header(a, image, n, o, 4 * i + 3);
      reinterpret_cast<float4*>(out)[i] = v;
    }
  } else {
    for (int i = tid; i < head; i += kRecThreads) out[i] = rec_header(a, image, n, o, i);
  }

  const bool affine = a.xform != nullptr;
  double t0 = 0, t1 = 0, t2 = 0, t3 = 0, t4 = 0, t5 = 0;
  if (affine) {
    const double* t = a.xform + (size_t)image * 6;
    t0 = t[0]; t1 = t[1]; t2 = t[2]; t3 = t[3]; t4 = t[4]; t5 = t[5];
  }
  float* kp = out + head;
  const int J = a.J, total = a.max_people * J;
  for (int e = tid; e < total; e += kRecThreads) {
    const int p = e / J;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (p < n) {
      const float* src = a.rows + ((size_t)(o + p) * J + (e - p * J)) * a.C;
      v.x = src[0]; v.y = src[1]; v.z = src[2]; v.w = src[3];
      if (affine) {
        // float64, two products, the left addition, the right one, one rounding (no contraction: -ffp-contract=off)
        const double x = (double)v.x, y = (double)v.y;
        v.x = (float)((t0 * x + t1 * y) + t2);
        v.y = (float)((t3 * x + t4 * y) + t5);
      }
    }
    if (kVec4) {
      reinterpret_cast<float4*>(kp)[e] = v;
    } else {
      kp[4 * (size_t)e] = v.x; kp[4 * (size_t)e + 1] = v.y; kp[4 * (size_t)e + 2] = v.z; kp[4 * (size_t)e + 3] = v.w;
    }
  }
}

}  // namespace
}  // namespace rtpe

using namespace rtpe;

extern "C" int rtpe_records_floats(int32_t J, int32_t max_people, size_t* floats) {
  RTPE_REQUIRE(floats && J > 0 && max_people > 0, "records_floats: bad argument");
  *floats = 2 + (size_t)max_people + (size_t)max_people * J * 4;
  return RTPE_OK;
}

extern "C" int rtpe_pack_records(const float* rows, int32_t C, const float* scores, const int32_t* counts,
                                 const int32_t* image_ids, const double* xform, int32_t N, int32_t J, int32_t cap,
                                 int32_t max_people, float* rec, size_t rec_bytes, void* stream) {
  RTPE_REQUIRE(rows && scores && counts && image_ids && rec, "pack_records: null rows, scores, counts, image_ids or rec");
  RTPE_REQUIRE(N > 0 && J > 0 && cap > 0 && max_people > 0,
               "pack_records: N = %d, J = %d, cap = %d, max_people = %d must be positive", N, J, cap, max_people);
  RTPE_REQUIRE(C >= 4, "pack_records: rows of %d columns, at least 4 (x, y, value, tag) are needed", C);
  RTPE_REQUIRE((long long)max_people * J <= 0x7fffffffLL / 4, "pack_records: max_people * J = %lld is too large",
               (long long)max_people * J);
  RecArgs a;
  a.floats = 2 + (size_t)max_people + (size_t)max_people * J * 4;
  RTPE_REQUIRE(rec_bytes / sizeof(float) / a.floats >= (size_t)N,
               "pack_records: rec of %zu bytes, %d records of %zu bytes are needed", rec_bytes, N,
               a.floats * sizeof(float));
  a.rows = rows; a.scores = scores; a.counts = counts; a.image_ids = image_ids; a.xform = xform; a.rec = rec;
  a.C = C; a.J = J; a.cap = cap; a.max_people = max_people;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const bool vec4 = (2 + max_people) % 4 == 0 && reinterpret_cast<uintptr_t>(rec) % 16 == 0;
  if (vec4)
    hipLaunchKernelGGL(pack_records_kernel<true>, dim3(N), dim3(kRecThreads), 0, s, a);
  else
    hipLaunchKernelGGL(pack_records_kernel<false>, dim3(N), dim3(kRecThreads), 0, s, a);
  RTPE_HIP_CHECK(hipGetLastError());
  return RTPE_OK;
}
