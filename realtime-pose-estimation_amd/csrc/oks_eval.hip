// COCO keypoint scoring of the device-resident records (include/rtpe_hip_oks.h; the rules: DESIGN.md section 4,
// "Scoring"): per record the stable score order of its people, the OKS matrix against the image's annotations in
// float64, and one sequential greedy matching per (threshold, area range) cell.  One 64-lane workgroup per record,
// the shape match_dev.hip has for grouping.  All arithmetic is written in the order of the float64 restatement
// (tests/scoring_restated.py) and compiled without contraction, so the two differ through exp() alone.
#include "rtpe_common.h"
#include "rtpe_hip_oks.h"

namespace rtpe {
namespace {

constexpr int kOksLanes = 64;
constexpr int kOksLdsFlags = 2048;      // matched-annotation bytes of all cells held in LDS
constexpr int kOksLdsG = 128;           // annotations whose flag words are held in LDS
constexpr double kOksSpacing = 2.220446049250313e-16;     // np.spacing(1)

struct OksArgs {
  const float* rec;
  const int32_t* gt_ids;
  const int32_t* gt_off;
  const double* gt_rows;
  const double* sigmas;
  const double* thr;
  const double* rngs;
  unsigned char* result;
  double* mat;                // scratch: (gt_cap * max_dets) doubles
  uint32_t* gflag;            //          (gt_cap) words: bit 0 crowd, bit 1 + r ignored in range r
  unsigned char* gtm;         //          (gt_cap * n_cells) bytes
  size_t rec_floats, row_bytes;
  int J, max_people, n_gt_images, n_thr, n_rng, max_dets, gt_cap;
};

__host__ __device__ inline size_t oks_row_bytes(int n_thr, int n_rng, int max_dets) {
  const size_t b = 8 + 4 * (size_t)max_dets + 2 * (size_t)n_thr * n_rng * max_dets;
  return (b + 7) / 8 * 8;
}

__host__ __device__ inline size_t oks_scratch_per_row(int n_thr, int n_rng, int max_dets) {
  return (size_t)max_dets * 8 + 4 + (size_t)n_thr * n_rng;
}

// OKS of one person (kp: J x 4 floats, x y value tag) against one annotation row
__device__ double oks_pair(const float* kp, const double* g, const double* sigmas, int J) {
  int k1 = 0;
  for (int j = 0; j < J; ++j) k1 += g[3 * j + 2] > 0.0;
  const double bx = g[51], by = g[52], bw = g[53], bh = g[54];
  const double x0 = bx - bw, x1 = bx + bw * 2.0, y0 = by - bh, y1 = by + bh * 2.0;
  const double area = g[55] + kOksSpacing;
  double sum = 0.0;
  int count = 0;
  for (int j = 0; j < J; ++j) {
    const double xd = (double)kp[4 * j], yd = (double)kp[4 * j + 1];
    double dx, dy;
    if (k1 > 0) {
      if (!(g[3 * j + 2] > 0.0)) continue;
      dx = xd - g[3 * j];
      dy = yd - g[3 * j + 1];
    } else {
      const double ax = x0 - xd, bx2 = xd - x1, ay = y0 - yd, by2 = yd - y1;
      dx = (ax > 0.0 ? ax : 0.0) + (bx2 > 0.0 ? bx2 : 0.0);
      dy = (ay > 0.0 ? ay : 0.0) + (by2 > 0.0 ? by2 : 0.0);
    }
    const double s2 = sigmas[j] * 2.0;
    const double e = (dx * dx + dy * dy) / (s2 * s2) / area / 2.0;
    sum += exp(-e);
    ++count;
  }
  return sum / (double)count;
}

__global__ __launch_bounds__(kOksLanes) void oks_eval_kernel(OksArgs a) {
  __shared__ double s_mat[RTPE_OKS_LDS_DOUBLES];
  __shared__ double s_darea[RTPE_OKS_MAX_DETS];
  __shared__ uint32_t s_gflag[kOksLdsG];
  __shared__ int s_order[RTPE_OKS_MAX_DETS];
  __shared__ unsigned char s_gtm[kOksLdsFlags];

  const int lane = threadIdx.x;
  const float* r = a.rec + (size_t)blockIdx.x * a.rec_floats;
  const int id = (int)r[0];
  int np = (int)r[1];
  np = np < 0 ? 0 : (np > a.max_people ? a.max_people : np);
  const int n_dt = np < a.max_dets ? np : a.max_dets;
  const int n_cells = a.n_thr * a.n_rng;

  // the image's annotations: rows [o0, o0 + G) of the table
  int lo = 0, hi = a.n_gt_images;
  while (lo < hi) {
    const int mid = lo + (hi - lo) / 2;
    if (a.gt_ids[mid] < id) lo = mid + 1; else hi = mid;
  }
  int o0 = 0, G = 0;
  if (lo < a.n_gt_images && a.gt_ids[lo] == id) {
    o0 = a.gt_off[lo];
    const int o1 = a.gt_off[lo + 1];
    if (o0 >= 0 && o1 > o0 && o1 <= a.gt_cap) G = o1 - o0; else o0 = 0;   // nothing beyond scratch, whatever the table says
  }

  // 1. stable rank by descending score
  s_order[lane] = 0;
  __syncthreads();
  for (int i = lane; i < np; i += kOksLanes) {
    const float si = r[2 + i];
    int rank = 0;
    for (int j = 0; j < np; ++j) {
      const float sj = r[2 + j];
      rank += (sj > si) || (sj == si && j < i);
    }
    if (rank < a.max_dets) s_order[rank] = i;
  }
  __syncthreads();
  const float* kpts = r + 2 + a.max_people;
  float score = 0.f;
  if (lane < n_dt) {
    const int p = s_order[lane];
    score = r[2 + p];
    const float* kp = kpts + (size_t)p * a.J * 4;
    double xmin = (double)kp[0], xmax = xmin, ymin = (double)kp[1], ymax = ymin;
    for (int j = 1; j < a.J; ++j) {
      const double x = (double)kp[4 * j], y = (double)kp[4 * j + 1];
      xmin = x < xmin ? x : xmin; xmax = x > xmax ? x : xmax;
      ymin = y < ymin ? y : ymin; ymax = y > ymax ? y : ymax;
    }
    s_darea[lane] = (xmax - xmin) * (ymax - ymin);
  }

  // where this record's working set lives: LDS while it fits, otherwise its block of scratch
  const bool small = (long long)a.max_dets * G <= RTPE_OKS_LDS_DOUBLES && (long long)n_cells * G <= kOksLdsFlags &&
                     G <= kOksLdsG;
  double* const gmat = a.mat + (size_t)o0 * a.max_dets;
  const double* const M = small ? s_mat : gmat;
  uint32_t* const gflag = small ? s_gflag : a.gflag + o0;
  unsigned char* const gtm = small ? s_gtm : a.gtm + (size_t)o0 * n_cells;

  for (int g = lane; g < G; g += kOksLanes) {
    const double* row = a.gt_rows + (size_t)(o0 + g) * RTPE_OKS_GT_ROW;
    const double area = row[55];
    const bool crowd = row[56] != 0.0;
    const bool ign = crowd || row[57] == 0.0;
    uint32_t f = crowd ? 1u : 0u;
    for (int q = 0; q < a.n_rng; ++q)
      if (ign || area < a.rngs[2 * q] || area > a.rngs[2 * q + 1]) f |= 2u << q;
    gflag[g] = f;
  }
  for (int i = lane; i < n_cells * G; i += kOksLanes) gtm[i] = 0;

  // 2. the OKS matrix (n_dt, G), always left in scratch as well (rtpe_hip_oks.h)
  for (int e = lane; e < n_dt * G; e += kOksLanes) {
    const int d = e / G, g = e - d * G;
    const double v = oks_pair(kpts + (size_t)s_order[d] * a.J * 4, a.gt_rows + (size_t)(o0 + g) * RTPE_OKS_GT_ROW,
                              a.sigmas, a.J);
    gmat[e] = v;
    if (small) s_mat[e] = v;
  }
  __syncthreads();

  // 3. one greedy matching per (threshold, range) cell; non-ignored annotations first, then the ignored ones
  unsigned char* out = a.result + (size_t)blockIdx.x * a.row_bytes;
  const size_t cells_bytes = (size_t)n_cells * a.max_dets;
  unsigned char* out_m = out + 8 + 4 * (size_t)a.max_dets;
  unsigned char* out_i = out_m + cells_bytes;
  for (int c = lane; c < n_cells; c += kOksLanes) {
    const int t = c / a.n_rng, q = c - t * a.n_rng;
    const double thr = a.thr[t], a_lo = a.rngs[2 * q], a_hi = a.rngs[2 * q + 1];
    const uint32_t ibit = 2u << q;
    unsigned char* gm = gtm + (size_t)c * G;
    for (int d = 0; d < a.max_dets; ++d) {
      unsigned char matched = 0, ignored = 0;
      if (d < n_dt) {
        double best = thr < 1.0 - 1e-10 ? thr : 1.0 - 1e-10;
        int m = -1;
        const double* Md = M + (size_t)d * G;
        for (int g = 0; g < G; ++g) {
          if ((gflag[g] & ibit) || gm[g]) continue;
          if (Md[g] < best) continue;
          best = Md[g]; m = g;
        }
        if (m < 0)
          for (int g = 0; g < G; ++g) {
            const uint32_t f = gflag[g];
            if (!(f & ibit) || (gm[g] && !(f & 1u))) continue;
            if (Md[g] < best) continue;
            best = Md[g]; m = g;
          }
        if (m >= 0) {
          matched = 1;
          ignored = (gflag[m] & ibit) ? 1 : 0;
          gm[m] = 1;
        } else {
          const double da = s_darea[d];
          ignored = (da < a_lo || da > a_hi) ? 1 : 0;
        }
      }
      out_m[(size_t)c * a.max_dets + d] = matched;
      out_i[(size_t)c * a.max_dets + d] = ignored;
    }
  }

  // header, scores and the padding behind the tables: every byte of the row
  if (lane == 0) {
    reinterpret_cast<int32_t*>(out)[0] = id;
    reinterpret_cast<int32_t*>(out)[1] = n_dt;
  }
  for (int d = lane; d < a.max_dets; d += kOksLanes) reinterpret_cast<float*>(out + 8)[d] = d < n_dt ? score : 0.f;
  for (size_t i = 8 + 4 * (size_t)a.max_dets + 2 * cells_bytes + lane; i < a.row_bytes; i += kOksLanes) out[i] = 0;
}

}  // namespace
}  // namespace rtpe

using namespace rtpe;

extern "C" int rtpe_oks_eval_bytes(int32_t n_records, int32_t gt_total, int32_t n_thr, int32_t n_rng,
                                   int32_t max_dets, size_t* result_bytes, size_t* scratch_bytes) {
  RTPE_REQUIRE(result_bytes && scratch_bytes, "oks_eval_bytes: null result_bytes or scratch_bytes");
  RTPE_REQUIRE(n_records > 0 && gt_total >= 0 && n_thr > 0 && n_rng > 0 && max_dets > 0,
               "oks_eval_bytes: n_records = %d, n_thr = %d, n_rng = %d, max_dets = %d must be positive, gt_total = %d "
               "not negative", n_records, n_thr, n_rng, max_dets, gt_total);
  RTPE_REQUIRE(max_dets <= RTPE_OKS_MAX_DETS && n_rng <= RTPE_OKS_MAX_RANGES && n_thr <= 4096,
               "oks_eval_bytes: max_dets = %d (at most %d), n_rng = %d (at most %d) or n_thr = %d (at most 4096) too large",
               max_dets, RTPE_OKS_MAX_DETS, n_rng, RTPE_OKS_MAX_RANGES, n_thr);
  *result_bytes = (size_t)n_records * oks_row_bytes(n_thr, n_rng, max_dets);
  const size_t s = (size_t)(gt_total > 0 ? gt_total : 1) * oks_scratch_per_row(n_thr, n_rng, max_dets);
  *scratch_bytes = (s + 7) / 8 * 8;
  return RTPE_OK;
}

extern "C" int rtpe_oks_eval(const float* rec, int32_t n_records, int32_t J, int32_t max_people,
                             const int32_t* gt_image_ids, const int32_t* gt_offsets, const double* gt_rows,
                             int32_t n_gt_images, const double* sigmas, const double* thresholds, int32_t n_thr,
                             const double* area_ranges, int32_t n_rng, int32_t max_dets, void* result,
                             size_t result_bytes, void* scratch, size_t scratch_bytes, void* stream) {
  RTPE_REQUIRE(rec && gt_image_ids && gt_offsets && gt_rows && sigmas && thresholds && area_ranges && result && scratch,
               "oks_eval: null rec, gt_image_ids, gt_offsets, gt_rows, sigmas, thresholds, area_ranges, result or scratch");
  RTPE_REQUIRE(n_records > 0 && J > 0 && max_people > 0 && n_gt_images > 0 && n_thr > 0 && n_rng > 0 && max_dets > 0,
               "oks_eval: n_records = %d, J = %d, max_people = %d, n_gt_images = %d, n_thr = %d, n_rng = %d, "
               "max_dets = %d must be positive", n_records, J, max_people, n_gt_images, n_thr, n_rng, max_dets);
  RTPE_REQUIRE(J <= 17, "oks_eval: J = %d, an annotation row holds 17 joints", J);
  RTPE_REQUIRE(max_dets <= max_people, "oks_eval: max_dets = %d exceeds max_people = %d", max_dets, max_people);
  RTPE_REQUIRE(max_dets <= RTPE_OKS_MAX_DETS && n_rng <= RTPE_OKS_MAX_RANGES && n_thr <= 4096,
               "oks_eval: max_dets = %d (at most %d), n_rng = %d (at most %d) or n_thr = %d (at most 4096) too large",
               max_dets, RTPE_OKS_MAX_DETS, n_rng, RTPE_OKS_MAX_RANGES, n_thr);
  RTPE_REQUIRE((long long)max_people * J <= 0x7fffffffLL / 4, "oks_eval: max_people * J = %lld is too large",
               (long long)max_people * J);
  OksArgs a;
  a.row_bytes = oks_row_bytes(n_thr, n_rng, max_dets);
  RTPE_REQUIRE(result_bytes / a.row_bytes >= (size_t)n_records,
               "oks_eval: result of %zu bytes, %d rows of %zu bytes are needed", result_bytes, n_records, a.row_bytes);
  const size_t per = oks_scratch_per_row(n_thr, n_rng, max_dets);
  RTPE_REQUIRE(scratch_bytes >= (per + 7) / 8 * 8, "oks_eval: scratch of %zu bytes, at least %zu are needed",
               scratch_bytes, (per + 7) / 8 * 8);
  RTPE_REQUIRE(reinterpret_cast<uintptr_t>(result) % 8 == 0 && reinterpret_cast<uintptr_t>(scratch) % 8 == 0,
               "oks_eval: result and scratch must be 8-byte aligned");
  const size_t cap = scratch_bytes / per;
  a.gt_cap = (int)(cap < 0x7fffffffULL ? cap : 0x7fffffffULL);
  a.rec = rec; a.gt_ids = gt_image_ids; a.gt_off = gt_offsets; a.gt_rows = gt_rows; a.sigmas = sigmas;
  a.thr = thresholds; a.rngs = area_ranges; a.result = static_cast<unsigned char*>(result);
  a.mat = static_cast<double*>(scratch);
  a.gflag = reinterpret_cast<uint32_t*>(a.mat + (size_t)a.gt_cap * max_dets);
  a.gtm = reinterpret_cast<unsigned char*>(a.gflag + a.gt_cap);
  a.rec_floats = 2 + (size_t)max_people + (size_t)max_people * J * 4;
  a.J = J; a.max_people = max_people; a.n_gt_images = n_gt_images; a.n_thr = n_thr; a.n_rng = n_rng;
  a.max_dets = max_dets;
  hipLaunchKernelGGL(oks_eval_kernel, dim3(n_records), dim3(kOksLanes), 0, reinterpret_cast<hipStream_t>(stream), a);
  RTPE_HIP_CHECK(hipGetLastError());
  return RTPE_OK;
}
