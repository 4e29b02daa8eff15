// Grouping of the top-K candidates into people on the GPU: a device restatement of match_image() of
// match_host.cpp (match_by_tag of the reference, group.py:26-97, with the Kuhn-Munkres procedure of the PyPI
// package `munkres`) for a batch of images, bit-identical to it.  match_host.cpp is the specification: every float
// operation, scan order and dictionary rule below is the one written there.
//
// Mapping: one wavefront (one 64-thread workgroup) per image, the joints in sequence.
//   * lane a owns candidate a of the joint and ROW a of the square cost matrix (n x n doubles, n = max(A, G) <= 64,
//     in LDS, row pitch odd: the rows are private to their lanes, LDS only serves as indexable per-lane memory);
//   * the zeros, stars and primes of a row are 64-bit masks in registers of the row's lane, the row and column covers
//     two wave-uniform 64-bit masks: find_zero is one ballot over the rows plus one lane read, "first star of a
//     column" one ballot, "first star / prime of a row" one lane read;
//   * the dictionary (keys, joint masks, tag lists and tag counts of the people of the image) lives in LDS, the people
//     rows in a per-image slice of a global buffer; address (person, joint, column c) is only ever written by lane c;
//   * a second kernel compacts the people of all images into ans / person_img / total with the prefix sum of counts.
// Nothing is waited for on the host and no value passes through it.
#include <math.h>

#include "rtpe_common.h"

namespace rtpe {
namespace {

typedef unsigned long long u64;

constexpr int kMatchMaxN = 64;      // K and max_num_people: one lane per candidate / person / row / column
constexpr int kMatchMaxJ = 32;      // joints: one bit each in a person's joint mask
constexpr int kMatchMaxD = 32;      // tag width: one lane each when a tag is copied
// LDS a workgroup may ask for: 1.5 x the 64 KiB a kernel gets without asking, which holds the largest tag (D = 32) at the
// decode's own sizes (J = 17, K = 30, max_num_people = 30: 85,440 bytes) and leaves 64 KiB of the CU's 160 to others
constexpr size_t kMatchMaxLds = 96 * 1024;
constexpr int kCompactPeople = 8;   // people per workgroup of the compaction kernel

struct MatchArgs {
  const float* tag_k;
  const int32_t* ind_k;
  const float* val_k;
  int J, K, D, w, max_people;
  double det_thr, tag_thr;
  int use_detection_val, ignore_too_much;
  float* rows;            // (N, cap_img, J, 3+D): rows of the joints named in jmask, the others are never written
  unsigned* jmask;        // (N, cap_img)
  int32_t* counts;        // (N), the caller's (possibly pinned host memory)
  int32_t* counts_dev;    // (N), the copy in device memory that the compaction reads
  int nmax, pitch, cap_img;
};

__device__ __forceinline__ u64 bit64(int i) { return 1ull << i; }
__device__ __forceinline__ int ctz64(u64 v) { return __builtin_ctzll(v); }

// the value of lane `l` (wave-uniform index)
__device__ __forceinline__ u64 lane_value(u64 v, int l) {
  const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)v, l);
  const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(v >> 32), l);
  return ((u64)hi << 32) | lo;
}

// OR of the values of lanes 0 .. n-1 (independent lane reads: no LDS round trips in a dependent chain)
__device__ __forceinline__ u64 wave_or(u64 v, int n) {
  u64 r = 0;
  for (int i = 0; i < n; ++i) r |= lane_value(v, i);
  return r;
}

__device__ __forceinline__ double wave_min(double v) {      // min of finite doubles: order-free
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const double u = __shfl_xor(v, o);
    v = u < v ? u : v;
  }
  return v;
}

// correctly rounded double square root: the compiler's expansion of sqrt (v_rsq_f64 + Goldschmidt steps), then
// Tuckerman's test with exact products: y = RN(sqrt(x))  <=>  y * pred(y) < x <= y * succ(y).
// (every x here is 0 or a sum of squares of float32 differences, >= 2^-298: the residuals do not underflow)
__device__ __forceinline__ double sqrt_rn(double x) {
  double y = __builtin_sqrt(x);
  if (x > 1e-200 && x < INFINITY) {
    const double ym = __longlong_as_double(__double_as_longlong(y) - 1);
    const double yp = __longlong_as_double(__double_as_longlong(y) + 1);
    if (__builtin_fma(y, ym, -x) >= 0.0) y = ym;
    else if (__builtin_fma(y, yp, -x) < 0.0) y = yp;
  }
  return y;
}

template <class F>
__device__ __forceinline__ float pairwise8_f32(F f, int n) {   // numpy contiguous float32 add.reduce
  if (n < 8) {
    float s = 0.f;
    for (int i = 0; i < n; ++i) s = s + f(i);
    return s;
  }
  float r0 = f(0), r1 = f(1), r2 = f(2), r3 = f(3), r4 = f(4), r5 = f(5), r6 = f(6), r7 = f(7);
  int i = 8;
  for (; i + 8 <= n; i += 8) {
    r0 = r0 + f(i); r1 = r1 + f(i + 1); r2 = r2 + f(i + 2); r3 = r3 + f(i + 3);
    r4 = r4 + f(i + 4); r5 = r5 + f(i + 5); r6 = r6 + f(i + 6); r7 = r7 + f(i + 7);
  }
  float s = ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7));
  for (; i < n; ++i) s = s + f(i);
  return s;
}

template <class F>
__device__ __forceinline__ double pairwise8_f64(F f, int n) {
  if (n < 8) {
    double s = 0.0;
    for (int i = 0; i < n; ++i) s = s + f(i);
    return s;
  }
  double r0 = f(0), r1 = f(1), r2 = f(2), r3 = f(3), r4 = f(4), r5 = f(5), r6 = f(6), r7 = f(7);
  int i = 8;
  for (; i + 8 <= n; i += 8) {
    r0 = r0 + f(i); r1 = r1 + f(i + 1); r2 = r2 + f(i + 2); r3 = r3 + f(i + 3);
    r4 = r4 + f(i + 4); r5 = r5 + f(i + 5); r6 = r6 + f(i + 6); r7 = r7 + f(i + 7);
  }
  double s = ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7));
  for (; i < n; ++i) s = s + f(i);
  return s;
}

// float64 distance of a candidate's tag to a person's mean tag (group.py:68-70: np.linalg.norm of the float64
// difference, i.e. sqrt of the pairwise sum of the squares)
__device__ __forceinline__ double tag_distance(const float* tag, const float* centre, int D) {
  const double ss = pairwise8_f64([&](int d) {
    const double df = (double)tag[d] - (double)centre[d];
    return df * df;
  }, D);
  return sqrt_rn(ss);
}

// Kuhn-Munkres on the n x n matrix whose row `lane` is `row` (lanes >= n idle); returns the stars of this lane's row.
// Step numbers and scan orders are those of Munkres::compute in match_host.cpp.
__device__ __forceinline__ u64 munkres_wave(double* row, int n, int lane) {
  const bool mine = lane < n;
  u64 zeros = 0, star = 0, prime = 0;
  u64 row_cov = 0, col_cov = 0;                             // wave-uniform
  // the row loops go in blocks of 8 independent LDS reads; a row's pitch covers the last block, entries at and
  // beyond n are read, never used (selects) and written back as they were
  if (mine) {                                               // step 1
    double m = row[0];
    for (int j0 = 0; j0 < n; j0 += 8) {
      double c[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) c[u] = row[j0 + u];
#pragma unroll
      for (int u = 0; u < 8; ++u) m = (j0 + u < n && c[u] < m) ? c[u] : m;
    }
    for (int j0 = 0; j0 < n; j0 += 8) {
      double c[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) c[u] = row[j0 + u];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const double d = j0 + u < n ? c[u] - m : c[u];
        row[j0 + u] = d;
        if (j0 + u < n && d == 0.0) zeros |= bit64(j0 + u);
      }
    }
  }
  for (int i = 0; i < n; ++i) {                             // step 2: rows in order, covers carried along
    const u64 z = lane_value(zeros, i) & ~col_cov;
    if (z) {
      const int j = ctz64(z);
      if (lane == i) star |= bit64(j);
      col_cov |= bit64(j);
    }
  }
  col_cov = 0;
  int z0r = 0, z0c = 0, step = 3;
  // the procedure ends after at most n augmentations with at most n step-6 rounds each; the bound only keeps
  // non-finite costs (NaN tags) from looping for ever
  for (int guard = 0; guard < 4 * n * n + 64; ++guard) {
    if (step == 3) {
      const u64 starred = wave_or(star, n);
      const int count = __builtin_popcountll(starred & ~col_cov);
      col_cov |= starred;
      if (count >= n) break;
      step = 4;
    } else if (step == 4) {
      int r = 0, q = 0;
      step = 6;
      for (int it = 0; it <= n; ++it) {                     // every round but the last covers one more row
        // find_zero(r, q): rows r, r+1, ... (mod n); within the row the LAST uncovered zero in the order
        // q, q+1, ... (mod n)
        const u64 rows_hit = __ballot(mine && !((row_cov >> lane) & 1) && (zeros & ~col_cov) != 0);
        if (!rows_hit) break;
        const u64 from = rows_hit & (~0ull << r);
        r = ctz64(from ? from : rows_hit);
        const u64 z = lane_value(zeros, r) & ~col_cov;
        const u64 below = z & (bit64(q) - 1);
        q = 63 - __builtin_clzll(below ? below : z);
        if (lane == r) { prime |= bit64(q); star &= ~bit64(q); }
        const u64 s = lane_value(star, r);
        if (!s) { z0r = r; z0c = q; step = 5; break; }
        q = ctz64(s);                                       // first star of the row
        row_cov |= bit64(r);
        col_cov &= ~bit64(q);
      }
    } else if (step == 5) {                                 // the searches see the marks before any flip
      u64 flipped = star;
      int pc = z0c;
      if (lane == z0r) flipped ^= bit64(pc);
      for (int it = 0; it <= n; ++it) {
        const u64 col_stars = __ballot((star >> pc) & 1);
        if (!col_stars) break;
        const int r = ctz64(col_stars);                     // first star of the column
        if (lane == r) flipped ^= bit64(pc);
        const u64 pm = lane_value(prime, r);
        if (!pm) break;
        pc = ctz64(pm);                                     // first prime of the row
        if (lane == r) flipped ^= bit64(pc);
      }
      star = flipped;
      prime = 0;
      row_cov = col_cov = 0;
      step = 3;
    } else {                                                // step 6
      double m = INFINITY;
      const u64 open_cols = ~col_cov & (n < 64 ? bit64(n) - 1 : ~0ull);
      if (mine && !((row_cov >> lane) & 1))
        for (int j0 = 0; j0 < n; j0 += 8) {
          double c[8];
#pragma unroll
          for (int u = 0; u < 8; ++u) c[u] = row[j0 + u];
#pragma unroll
          for (int u = 0; u < 8; ++u) m = (j0 + u < n && ((open_cols >> (j0 + u)) & 1) && c[u] < m) ? c[u] : m;
        }
      m = wave_min(m);
      if (mine) {
        const bool rc = (row_cov >> lane) & 1;
        zeros = 0;
        for (int j0 = 0; j0 < n; j0 += 8) {
          double c[8];
#pragma unroll
          for (int u = 0; u < 8; ++u) c[u] = row[j0 + u];
#pragma unroll
          for (int u = 0; u < 8; ++u) {
            const int j = j0 + u;
            double d = c[u];
            if (j < n) {
              if (rc) d += m;
              if ((open_cols >> j) & 1) d -= m;
            }
            row[j] = d;
            if (j < n && d == 0.0) zeros |= bit64(j);
          }
        }
      }
      step = 4;
    }
  }
  return star;
}

__global__ void __launch_bounds__(64) match_by_tag_kernel(const MatchArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char match_lds[];
  const int lane = threadIdx.x, img = blockIdx.x;
  const int J = a.J, K = a.K, D = a.D, R = 3 + a.D, MP = a.max_people;
  double* cost = reinterpret_cast<double*>(match_lds);
  float* cand = reinterpret_cast<float*>(cost + (size_t)a.nmax * a.pitch);   // (K, R): x, y, val, tag
  float* centres = cand + K * R;                                             // (MP, D)
  float* tags = centres + MP * D;                                            // (MP, J, D): tag_dict of the first MP
  int* n_tags = reinterpret_cast<int*>(tags + (size_t)MP * J * D);           // (MP)
  float* keys = reinterpret_cast<float*>(n_tags + MP);                       // (cap_img): tag[0] of the founder
  unsigned* jm = reinterpret_cast<unsigned*>(keys + a.cap_img);              // (cap_img): joints whose row was written
  const float* tag_k = a.tag_k + (size_t)img * J * K * D;
  const int32_t* ind_k = a.ind_k + (size_t)img * J * K;
  const float* val_k = a.val_k + (size_t)img * J * K;
  float* rows = a.rows + (size_t)img * a.cap_img * J * R;
  double* my_row = cost + (size_t)lane * a.pitch;
  int np = 0;                                               // people so far (wave-uniform)

  // put(): the dict semantics of match_image - found by == on the float key, first match in insertion order;
  // an existing key gets row j overwritten and its tag list RESET to this one tag
  auto put = [&](int j, int c) {
    const float* cr = cand + c * R;
    const float key = cr[3];
    int pi = -1;
    for (int base = 0; base < np; base += 64) {
      const int p = base + lane;
      const u64 hit = __ballot(p < np && keys[p] == key);
      if (hit) { pi = base + ctz64(hit); break; }
    }
    if (pi < 0) {
      if (np >= a.cap_img) return;                          // (unreachable: every candidate founds at most one person)
      pi = np++;
      if (lane == 0) { keys[pi] = key; jm[pi] = 0; }
    }
    if (lane < R) rows[((size_t)pi * J + j) * R + lane] = cr[lane];
    if (lane == 0) jm[pi] |= 1u << j;
    if (pi < MP) {
      if (lane < D) tags[(size_t)pi * J * D + lane] = cr[3 + lane];
      if (lane == 0) n_tags[pi] = 1;
    }
    __syncthreads();
  };

  for (int j = 0; j < J; ++j) {
    __syncthreads();
    const float v = lane < K ? val_k[j * K + lane] : 0.f;
    const bool keep = lane < K && (double)v > a.det_thr;
    const u64 kept = __ballot(keep);
    const int A = __builtin_popcountll(kept);
    if (A == 0) continue;
    if (keep) {
      float* cr = cand + __builtin_popcountll(kept & (bit64(lane) - 1)) * R;
      const int ind = ind_k[j * K + lane];
      cr[0] = (float)(ind % a.w);                           // integers below 2^24: exact in float32
      cr[1] = (float)(ind / a.w);
      cr[2] = v;
      for (int d = 0; d < D; ++d) cr[3 + d] = tag_k[((size_t)j * K + lane) * D + d];
    }
    __syncthreads();
    if (j == 0 || np == 0) {
      for (int c = 0; c < A; ++c) put(j, c);
      continue;
    }
    const int G = np < MP ? np : MP;
    if (a.ignore_too_much && G == MP) continue;
    if (lane < G) {                                         // mean tag of person `lane`, numpy's float32 order
      const float* t = tags + (size_t)lane * J * D;
      const int nt = n_tags[lane];
      for (int d = 0; d < D; ++d) {
        float s;
        if (D == 1) {
          s = pairwise8_f32([&](int i) { return t[i]; }, nt);
        } else {
          s = 0.f;
          for (int i = 0; i < nt; ++i) s = s + t[i * D + d];
        }
        centres[lane * D + d] = s / (float)nt;
      }
    }
    __syncthreads();
    const int n = A > G ? A : G;
    if (lane < n) {
      if (lane < A) {
        const float* cr = cand + lane * R;
        for (int g = 0; g < G; ++g) {
          const double dd = tag_distance(cr + 3, centres + g * D, D);
          my_row[g] = a.use_detection_val ? __builtin_rint(dd) * 100.0 - (double)cr[2] : dd;
        }
        for (int g = G; g < n; ++g) my_row[g] = 1e10;
      } else {
        for (int g = 0; g < n; ++g) my_row[g] = 0.0;
      }
    }
    const u64 star = munkres_wave(my_row, n, lane);
    for (int r = 0; r < A; ++r) {                           // the pairs in row-major order
      u64 s = lane_value(star, r);
      while (s) {
        const int q = ctz64(s);
        s &= s - 1;
        bool joined = false;
        if (q < G) joined = tag_distance(cand + r * R + 3, centres + q * D, D) < a.tag_thr;
        if (joined) {
          const int nt = n_tags[q];
          if (lane < R) rows[((size_t)q * J + j) * R + lane] = cand[r * R + lane];
          if (nt < J && lane < D) tags[((size_t)q * J + nt) * D + lane] = cand[r * R + 3 + lane];
          __syncthreads();
          if (lane == 0) { jm[q] |= 1u << j; n_tags[q] = nt + 1; }
          __syncthreads();
        } else {
          put(j, r);
        }
      }
    }
  }
  __syncthreads();
  if (lane == 0) { a.counts[img] = np; a.counts_dev[img] = np; }
  unsigned* jmask = a.jmask + (size_t)img * a.cap_img;
  for (int p = lane; p < np; p += 64) jmask[p] = jm[p];
}

// people of image n follow those of image n-1; rows of joints a person never got are zero
__global__ void __launch_bounds__(256) match_compact_kernel(const float* rows, const unsigned* jmask,
                                                            const int32_t* counts, int N, int J, int R, int cap_img,
                                                            float* ans, int cap, int32_t* person_img,
                                                            int32_t* total) {
  __shared__ int base_s;
  const int n = blockIdx.y;
  const int count = counts[n];
  const bool last = blockIdx.x == 0 && n == N - 1;          // this workgroup also writes the total
  if (blockIdx.x * kCompactPeople >= count && !last) return;
  if (threadIdx.x == 0) {
    int b = 0;
    for (int m = 0; m < n; ++m) b += counts[m];
    base_s = b;
    if (last) *total = b + count;
  }
  __syncthreads();
  const int base = base_s;
  const int p0 = blockIdx.x * kCompactPeople;
  const int len = J * R;
  for (int e = threadIdx.x; e < kCompactPeople * len; e += 256) {
    const int p = p0 + e / len, c = e % len;
    if (p >= count || base + p >= cap) continue;
    const size_t src = ((size_t)n * cap_img + p);
    const bool have = (jmask[src] >> (c / R)) & 1;
    ans[(size_t)(base + p) * len + c] = have ? rows[src * len + c] : 0.f;
    if (c == 0) person_img[base + p] = n;
  }
}

static int match_pitch(int nmax) { return ((nmax + 7) & ~7) | 1; }   // whole blocks of 8, odd: rows on different banks

static size_t match_lds_bytes(int J, int K, int D, int max_people) {
  const int nmax = K > max_people ? K : max_people;
  const int pitch = match_pitch(nmax);
  const size_t cap_img = (size_t)J * K;
  return (size_t)nmax * pitch * sizeof(double) + ((size_t)K * (3 + D) + (size_t)max_people * D +
         (size_t)max_people * J * D + max_people + 2 * cap_img) * sizeof(float);
}

static size_t match_scratch(int N, int J, int K, int D) {
  return (size_t)N * J * K * ((size_t)J * (3 + D) * sizeof(float) + sizeof(unsigned)) + (size_t)N * sizeof(int32_t);
}

static int match_check_dims(const char* what, int N, int J, int K, int D) {
  RTPE_REQUIRE(N > 0 && J > 0 && K > 0 && D > 0, "%s: bad argument", what);
  RTPE_REQUIRE(K <= kMatchMaxN, "%s: K = %d candidates per joint, the device matcher takes at most %d", what, K,
               kMatchMaxN);
  RTPE_REQUIRE(J <= kMatchMaxJ, "%s: J = %d joints, the device matcher takes at most %d", what, J, kMatchMaxJ);
  RTPE_REQUIRE(D <= kMatchMaxD, "%s: D = %d tag values, the device matcher takes at most %d", what, D, kMatchMaxD);
  RTPE_REQUIRE(N <= 65535, "%s: N = %d images, the device matcher takes at most 65535", what, N);
  return RTPE_OK;
}

}  // namespace
}  // namespace rtpe

using namespace rtpe;

extern "C" int rtpe_match_by_tag_dev_scratch_bytes(int32_t N, int32_t J, int32_t K, int32_t D, size_t* bytes) {
  RTPE_REQUIRE(bytes, "match_by_tag_dev_scratch_bytes: bad argument");
  const int rc = match_check_dims("match_by_tag_dev_scratch_bytes", N, J, K, D);
  if (rc != RTPE_OK) return rc;
  *bytes = match_scratch(N, J, K, D);
  return RTPE_OK;
}

extern "C" int rtpe_match_by_tag_dev(const float* tag_k, const int32_t* ind_k, const float* val_k, int32_t N,
                                     int32_t J, int32_t K, int32_t D, int32_t w, int32_t max_num_people,
                                     double detection_threshold, double tag_threshold, int32_t use_detection_val,
                                     int32_t ignore_too_much, float* ans, int32_t cap, int32_t* person_img,
                                     int32_t* counts, int32_t* total, void* scratch, size_t scratch_bytes,
                                     void* stream) {
  RTPE_REQUIRE(tag_k && ind_k && val_k && ans && person_img && counts && total && w > 0,
               "match_by_tag_dev: bad argument");
  const int rc = match_check_dims("match_by_tag_dev", N, J, K, D);
  if (rc != RTPE_OK) return rc;
  RTPE_REQUIRE(max_num_people >= 1 && max_num_people <= kMatchMaxN,
               "match_by_tag_dev: max_num_people = %d, the device matcher takes 1 to %d", max_num_people, kMatchMaxN);
  RTPE_REQUIRE((long long)cap >= (long long)N * J * K,
               "match_by_tag_dev: room for %d people, %lld (N*J*K: every candidate may found one) are needed", cap,
               (long long)N * J * K);
  const size_t lds = match_lds_bytes(J, K, D, max_num_people);
  RTPE_REQUIRE(lds <= kMatchMaxLds,
               "match_by_tag_dev: J = %d, K = %d, D = %d, max_num_people = %d need %zu bytes of LDS, the limit is %zu",
               J, K, D, max_num_people, lds, kMatchMaxLds);
  RTPE_REQUIRE(scratch && scratch_bytes >= match_scratch(N, J, K, D), "match_by_tag_dev: scratch too small");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  MatchArgs a;
  a.tag_k = tag_k; a.ind_k = ind_k; a.val_k = val_k;
  a.J = J; a.K = K; a.D = D; a.w = w; a.max_people = max_num_people;
  a.det_thr = detection_threshold; a.tag_thr = tag_threshold;
  a.use_detection_val = use_detection_val; a.ignore_too_much = ignore_too_much;
  a.cap_img = J * K;
  a.rows = reinterpret_cast<float*>(scratch);
  a.jmask = reinterpret_cast<unsigned*>(a.rows + (size_t)N * a.cap_img * J * (3 + D));
  a.counts = counts;
  a.counts_dev = reinterpret_cast<int32_t*>(a.jmask + (size_t)N * a.cap_img);
  a.nmax = K > max_num_people ? K : max_num_people;
  a.pitch = match_pitch(a.nmax);
  static unsigned long long attr_mask = 0;                  // beyond 64 KiB a kernel has to be allowed its dynamic LDS
  if (lds > 64 * 1024 && first_use_on_device(&attr_mask))
    RTPE_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(match_by_tag_kernel),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)kMatchMaxLds));
  hipLaunchKernelGGL(match_by_tag_kernel, dim3(N), dim3(64), lds, s, a);
  RTPE_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(match_compact_kernel, dim3((a.cap_img + kCompactPeople - 1) / kCompactPeople, N), dim3(256), 0, s,
                     a.rows, a.jmask, a.counts_dev, N, J, 3 + D, a.cap_img, ans, cap, person_img, total);
  RTPE_HIP_CHECK(hipGetLastError());
  return RTPE_OK;
}
