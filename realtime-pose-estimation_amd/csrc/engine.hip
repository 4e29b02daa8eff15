// Program executor: runs the flat op list that the Python module tree compiles
// itself into (rtpe/third_party/pose_higher_hrnet.py of this repo) with the
// kernels of conv_mfma.hip / elementwise.hip.  Owns only the packed weights.
#include <stdarg.h>

#include <chrono>
#include <mutex>
#include <map>
#include <tuple>
#include <vector>

#include "rtpe_common.h"

namespace rtpe {

static thread_local std::string g_err;

void set_error(const char* fmt, ...) {
  char buf[1024];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  g_err = buf;
}

int hip_fail(hipError_t e, const char* what, const char* file, int line) {
  set_error("HIP error %d (%s) at %s:%d: %s", (int)e, hipGetErrorString(e), file, line, what);
  return RTPE_E_HIP;
}

struct OpState {
  rtpe_op_desc d;
  ConvGeom geom[4];   // 1 for CONV, 4 parity classes for DECONV
  ConvPlan plan[4];
  size_t w_dev_off[4];  // byte offsets in the device weight arena
  size_t ab_dev_off;    // alpha then beta, fp32[cout_pad]
  int n_geom;
  int fuse;             // 1: head of a fused BasicBlock (this conv + the next run as one kernel), 2: its second conv
  int pair;             // 1: head of a 1x1 pair (conv_pair.hip: launched with the next op), 2: its tail
  int proj_head;        // > 0: this conv is the skip projection that the 1x1 pair with head ops[proj_head] may compute itself
  int proj_op;          // on that head: the projection's op index (else -1)
  int stem2;            // 1: the stem op whose conv1 runs together with the next op's conv2 (stem_fused.hip), 2: that conv op
  int s2g;              // n > 1: first of n neighbouring 3x3 stride-2 convs from the SAME 48-channel input that run as one launch
                        // (conv48s2.hip: the input is read once), -1: one of the others
};

}  // namespace rtpe

using namespace rtpe;

// ---- routing: which launch computes each op of one forward ------------------------------------------------------------
// route_ops() decides it in one pass over the ops, from the options as they are at that moment; launch_op() launches what the
// routes say, rtpe_hrnet_op_tile reports them, the per-op times and the autotuner read them.  A new fused launch is one more
// kind here: its conditions in route_ops(), its case in launch_op(), its mark in route_label().
enum {
  kRouteNone = 0,                                        // no conv (an elementwise / student op)
  kRouteTile, kRouteStream, kRouteDirect, kRouteConv64,  // conv_launch on tile[k], one launch per parity class: ConvTile::kind 0 / 2 / 4 / 5
  kRouteHead,                                            // conv_direct.hip's head kernel (option "head_direct")
  kRouteS2,                                              // conv48s2.hip, a launch of its own (option "conv48s2")
  kRouteS2Group,                                         // conv48s2.hip, this op and the by - 1 behind it as one launch
  kRouteDeconvMerged, kRouteDeconv48,                    // the 4 classes of a transposed conv as one grid on tile[0] / on deconv48.hip
  kRoutePairHead, kRoutePairTail, kRoutePairProj,        // conv_pair.hip: ONE launch at the tail; by = the tail (head, projection) / the head (tail)
  kRouteBlock,                                           // conv_block.hip: this conv and the next one
  kRouteStemFused, kRouteStemConv1, kRouteStemPlain,     // stem_fused.hip with the next op / its conv1 code alone ("fused_stem" = 2) / the VALU kernel
  kRouteDoneBy                                           // computed by the launch at op `by` (a block's second conv, the stem's conv2, a group's others)
};
// the numbers a trace reports (rtpe_hip_trace.h): a kind added in the middle of the list must not renumber them silently
static_assert(kRouteTile == RTPE_ROUTE_TILE && kRouteHead == RTPE_ROUTE_HEAD && kRouteS2 == RTPE_ROUTE_S2 && kRouteS2Group == RTPE_ROUTE_S2_GROUP &&
              kRouteDeconvMerged == RTPE_ROUTE_DECONV_MERGED && kRoutePairHead == RTPE_ROUTE_PAIR_HEAD && kRoutePairTail == RTPE_ROUTE_PAIR_TAIL &&
              kRoutePairProj == RTPE_ROUTE_PAIR_PROJ && kRouteBlock == RTPE_ROUTE_BLOCK && kRouteStemFused == RTPE_ROUTE_STEM_FUSED &&
              kRouteStemConv1 == RTPE_ROUTE_STEM_CONV1 && kRouteStemPlain == RTPE_ROUTE_STEM_PLAIN && kRouteDoneBy == RTPE_ROUTE_DONE_BY,
              "rtpe_hip_trace.h names other route numbers");

static void trace_put(std::vector<int32_t>* tr, int kind, int a, int b, int c = 0, int d = 0) {
  const int32_t r[RTPE_TRACE_INTS] = {kind, a, b, c, d};
  tr->insert(tr->end(), r, r + RTPE_TRACE_INTS);
}

struct Route {
  int how, by;
  ConvTile tile[4];     // conv ops: the launch shape of every parity class, after the rules that override a tuned or default one
};

struct rtpe_record {    // rtpe_hrnet_forward_record: the events of one forward and the routes that say which of them exist
  std::vector<hipEvent_t> ev;
  std::vector<Route> routes;
};

struct rtpe_hrnet {
  int device;
  std::vector<OpState> ops;
  // autotuned launch shapes: (N, H, W) -> one ConvTile per (op, parity class); nt == 0 = not tuned
  std::map<std::tuple<int, int, int>, std::vector<ConvTile>> tuned;
  std::map<int, rtpe_record> records;                // rtpe_hrnet_forward_record, by slot
  std::vector<rtpe_tensor_desc> tensors;
  // tensors that MAY be kept plane-major ([C/48][N][H][W][48] instead of NHWC): C >= 96 and every op that
  // touches them is a 3x3 stride-1 conv the streaming kernel runs (the inner tensors of a BasicBlock chain).
  // A 48-channel block is then one contiguous row per image row instead of 96 bytes of every 2C: the
  // kernel's stores, residual loads and halo DMA move whole cache lines.  Decided per run (see run()).
  std::vector<char> plane_ok;
  int n_slots;
  char* arena;        // device: packed weights + affine params
  size_t arena_bytes;
  int n_preds, n_refined;
  // parallel regions (rtpe_op_desc::lane / region): internal streams for lanes 1..3 and one event per op whose output
  // another lane reads, created on first use; wait_ops[i] = ops of other lanes whose output op i reads
  // THREADS: the lane streams and events are state of the handle; a forward with lanes on holds lane_mu from the creation
  // of that state (first such forward) to the join of its last region, so two host threads on one handle enqueue their
  // lane regions one after the other (their kernels still overlap on the GPU when they use different streams)
  std::mutex lane_mu;
  hipStream_t lane_stream[4] = {nullptr, nullptr, nullptr, nullptr};
  std::vector<hipEvent_t> op_event;
  std::vector<char> needs_event;
  std::vector<std::vector<int>> wait_ops;
  hipEvent_t fork_event = nullptr;
  bool has_regions = false;
  std::vector<int32_t> trace;     // what the last forward with RTPE_FWD_TRACE enqueued (rtpe_hip_trace.h), 5 integers per record
  bool any_size = false;     // rtpe_hrnet_set_any_size: ragged shapes (a side that is no multiple of 32) are taken, on the general paths
};

static size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

namespace rtpe {
static int g_options[kNumOptions] = {-1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1};   // -1: not set, take the environment's value
static const char* const kOptionNames[kNumOptions] = {"block_ring", "block_pc", "direct_1x1", "lanes", "tile_dma", "pair_1x1", "fused_stem", "conv64", "head_direct", "deconv48", "conv48s2", "pair_proj"};
static const char* const kOptionEnv[kNumOptions] = {"RTPE_BLOCK_RING", "RTPE_BLOCK_PC", "RTPE_DIRECT_1X1", "RTPE_LANES", "RTPE_TILE_DMA", "RTPE_PAIR_1X1", "RTPE_FUSED_STEM", "RTPE_CONV64", "RTPE_HEAD_DIRECT", "RTPE_DECONV48", "RTPE_CONV48S2", "RTPE_PAIR_PROJ"};
static const int kOptionDefault[kNumOptions] = {0, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1};
int get_option(int key) {
  int v = __atomic_load_n(&g_options[key], __ATOMIC_RELAXED);
  if (v < 0) {
    v = kOptionEnv[key][0] ? env_int(kOptionEnv[key], kOptionDefault[key]) : kOptionDefault[key];
    __atomic_store_n(&g_options[key], v, __ATOMIC_RELAXED);
  }
  return v;
}
}  // namespace rtpe

extern "C" int rtpe_set_option(const char* name, int32_t value) {
  RTPE_REQUIRE(name != nullptr && value >= 0, "set_option: bad argument");
  for (int k = 0; k < kNumOptions; ++k)
    if (kOptionNames[k][0] && strcmp(name, kOptionNames[k]) == 0) {
      __atomic_store_n(&g_options[k], (int)value, __ATOMIC_RELAXED);
      return RTPE_OK;
    }
  set_error("set_option: unknown option '%s'", name);
  return RTPE_E_INVALID;
}

extern "C" int rtpe_get_option(const char* name, int32_t* value) {
  RTPE_REQUIRE(name != nullptr && value != nullptr, "get_option: null argument");
  for (int k = 0; k < kNumOptions; ++k)
    if (kOptionNames[k][0] && strcmp(name, kOptionNames[k]) == 0) {
      *value = get_option(k);
      return RTPE_OK;
    }
  set_error("get_option: unknown option '%s'", name);
  return RTPE_E_INVALID;
}

extern "C" const char* rtpe_last_error_string(void) { return g_err.c_str(); }
extern "C" int rtpe_version(void) { return 4; }   // 4: no "stream_pc" / kind 3; 3: 11 integers per tuned record; 2: rtpe_op_desc has lane / region, rtpe_hrnet_forward_flags
extern "C" int rtpe_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

// ---- rtpe_hrnet_create: one function per pass over the ops, called in this order.  Together they produce every OpState field
// and every table of the handle that a forward reads ---------------------------------------------------------------------

// plans + arena layout: the op descriptors checked, a plan per conv class, the place of every op's weights in the arena
static int plan_ops(rtpe_hrnet* h, const rtpe_op_desc* ops, int n_ops, size_t weights_bytes) {
  const int n_tensors = (int)h->tensors.size();
  size_t off = 0;
  h->ops.resize(n_ops);
  for (int i = 0; i < n_ops; ++i) {
    OpState& o = h->ops[i];
    o.d = ops[i];
    o.n_geom = 0;
    const rtpe_op_desc& d = o.d;
    auto bad_t = [&](int t) { return t < 0 || t >= n_tensors; };
    if (d.kind != RTPE_OP_FUSE && d.kind != RTPE_OP_STEM && d.kind != RTPE_OP_AUX_PACK && bad_t(d.in_t)) {
      set_error("op %d: bad input tensor", i); return RTPE_E_INVALID;
    }
    if (bad_t(d.out_t) && !(d.flags & RTPE_F_NO_NHWC)) {
      set_error("op %d: bad output tensor", i); return RTPE_E_INVALID;
    }
    if (d.flags & RTPE_F_OUT_PREDS) h->n_preds = d.cout;
    if (d.flags & RTPE_F_OUT_REFINED) h->n_refined = d.cout;
    if (d.kind == RTPE_OP_CONV || d.kind == RTPE_OP_DECONV) {
      o.n_geom = d.kind == RTPE_OP_DECONV ? 4 : 1;
      for (int k = 0; k < o.n_geom; ++k) {
        o.geom[k] = ConvGeom{d.cin, d.cout, d.ksize, d.stride, d.kind == RTPE_OP_DECONV ? k : -1,
                             (d.flags & RTPE_F_F32) ? 4 : 2, d.reserved[1] > 0 ? d.reserved[1] : 1};
        o.plan[k] = conv_make_plan(o.geom[k]);
        o.w_dev_off[k] = off;
        off = align_up(off + o.plan[k].packed_bytes, 256);
      }
      o.ab_dev_off = off;
      off = align_up(off + 2 * sizeof(float) * o.plan[0].cout_pad, 256);
      const size_t wbytes = (size_t)d.cin * d.cout * d.ksize * d.ksize * ((d.flags & RTPE_F_F32) ? 4 : 2);
      if (d.w_off < 0 || (size_t)d.w_off + wbytes > weights_bytes ||
          d.ab_off < 0 || (size_t)d.ab_off + 8 * (size_t)d.cout > weights_bytes) {
        set_error("op %d: weight offsets out of range", i); return RTPE_E_INVALID;
      }
    } else if (d.kind == RTPE_OP_STEM) {
      o.w_dev_off[0] = off;
      off = align_up(off + 27 * 64 * 4, 256);
      o.ab_dev_off = off;
      off = align_up(off + 2 * sizeof(float) * 64, 256);
      if (d.cout != 64 || d.cin != 3) { set_error("stem must be 3->64"); return RTPE_E_INVALID; }
    } else if (d.kind == RTPE_OP_FUSE) {
      if (d.n_terms < 1 || d.n_terms > 4) { set_error("op %d: fuse terms", i); return RTPE_E_INVALID; }
    } else if (d.kind == RTPE_OP_SE) {
      const size_t wbytes = ((size_t)d.cout * d.cin * 2 + d.cout + d.cin) * 4;
      if (d.w_off < 0 || (size_t)d.w_off + wbytes > weights_bytes) {
        set_error("op %d: SE weights out of range", i); return RTPE_E_INVALID;
      }
      o.w_dev_off[0] = off;
      off = align_up(off + wbytes, 256);
    } else if (d.kind == RTPE_OP_CAST || d.kind == RTPE_OP_AVGPOOL || d.kind == RTPE_OP_CAM_COMBINE ||
               d.kind == RTPE_OP_SIGMOID_ADD || d.kind == RTPE_OP_RESIZE || d.kind == RTPE_OP_GATE_MUL) {
      if ((d.kind == RTPE_OP_CAM_COMBINE && (bad_t(d.res_t) || bad_t(d.term_t[0]))) ||
          ((d.kind == RTPE_OP_SIGMOID_ADD || d.kind == RTPE_OP_GATE_MUL) && bad_t(d.res_t))) {
        set_error("op %d: missing operand tensor", i); return RTPE_E_INVALID;
      }
    } else if (d.kind == RTPE_OP_AUX_PACK) {
      const rtpe_tensor_desc& t = h->tensors[d.out_t];      // fp32: rows of (r, g, b, 0); fp16 (no RTPE_F_F32): (r, g, b, 0 x 5)
      if ((d.flags & RTPE_F_F32) ? (t.reserved != 4 || t.channels < 4) : (t.reserved == 4 || t.channels < 8)) {
        set_error("op %d: the packed second input must be an fp32 tensor of >= 4 channels (fp16 form: an fp16 tensor of >= 8)", i);
        return RTPE_E_INVALID;
      }
    } else {
      set_error("op %d: unknown kind %d", i, d.kind); return RTPE_E_INVALID;
    }
  }
  h->arena_bytes = off;
  return RTPE_OK;
}

// BasicBlock fusion (conv_block.hip): conv 48->48 k3 s1 +relu, then conv 48->48 k3 s1 +residual(+relu)
// whose residual is the first conv's input and whose input is read by nobody else
static void mark_blocks(rtpe_hrnet* h) {
  static const int fuse_blocks = getenv("RTPE_FUSE_BLOCKS") ? atoi(getenv("RTPE_FUSE_BLOCKS")) : 1;
  for (size_t i = 0; fuse_blocks && i + 2 < h->ops.size(); ++i) {     // (the last op keeps its own event)
    OpState& a1 = h->ops[i];
    OpState& a2 = h->ops[i + 1];
    const rtpe_op_desc& d1 = a1.d;
    const rtpe_op_desc& d2 = a2.d;
    const int plain = RTPE_F_RELU | RTPE_F_ROUND_CONV;
    if (a1.fuse || d1.kind != RTPE_OP_CONV || d2.kind != RTPE_OP_CONV) continue;
    if (d1.cin != 48 || d1.cout != 48 || d2.cin != 48 || d2.cout != 48 || d1.ksize != 3 || d2.ksize != 3 ||
        d1.stride != 1 || d2.stride != 1 || d1.flags != plain || d2.flags != plain || d1.res_t >= 0 ||
        d2.res_t != d1.in_t || d2.res_coff != d1.in_coff || d2.in_t != d1.out_t || d2.in_coff != d1.out_coff ||
        d1.reserved[1] > 1 || d2.reserved[1] > 1 || h->tensors[d1.in_t].reserved == 4 || d2.out_t == d1.in_t)
      continue;
    bool other_reader = false;                       // the intermediate tensor must die inside the block
    for (size_t k = 0; k < h->ops.size() && !other_reader; ++k) {
      if (k == i + 1) continue;
      const rtpe_op_desc& dk = h->ops[k].d;
      if (k > i && (dk.in_t == d1.out_t || dk.res_t == d1.out_t)) other_reader = true;
      for (int t = 0; t < dk.n_terms && k > i; ++t) other_reader |= dk.term_t[t] == d1.out_t;
    }
    if (other_reader) continue;
    a1.fuse = 1;
    a2.fuse = 2;
  }
}

// fused stem (stem_fused.hip): the stem op, then conv 64->64 k3 s2 (+relu) that is the only reader of its output
static void mark_stems(rtpe_hrnet* h) {
  for (OpState& o : h->ops) o.stem2 = 0;
  for (size_t i = 0; i + 1 < h->ops.size(); ++i) {
    OpState& a1 = h->ops[i];
    OpState& a2 = h->ops[i + 1];
    const rtpe_op_desc &d1 = a1.d, &d2 = a2.d;
    if (d1.kind != RTPE_OP_STEM || (d1.flags & RTPE_F_F32) || d2.kind != RTPE_OP_CONV || a2.fuse || a2.n_geom != 1) continue;
    const ConvPlan& p2 = a2.plan[0];
    if (d2.cin != 64 || d2.cout != 64 || d2.ksize != 3 || d2.stride != 2 || d2.res_t >= 0 || d2.n_terms != 0 ||
        (d2.flags & ~(RTPE_F_RELU | RTPE_F_ROUND_CONV)) || d2.in_t != d1.out_t || d2.in_coff != 0 || d1.out_coff != 0 ||
        d2.reserved[1] > 1 || d2.reserved[2] > 0 || d2.out_t == d1.out_t || h->tensors[d1.out_t].channels != 64 ||
        h->tensors[d2.out_t].channels - d2.out_coff < 64 || d1.lane != d2.lane || d1.region != d2.region ||
        p2.mt != 4 || p2.cc != 64 || p2.n_cchunks != 1 || p2.kc != 18 || p2.n_cb != 1 || p2.esize != 2)
      continue;
    bool other_reader = false;
    for (size_t k = i + 2; k < h->ops.size() && !other_reader; ++k) {
      const rtpe_op_desc& dk = h->ops[k].d;
      if (dk.in_t == d1.out_t || dk.res_t == d1.out_t) other_reader = true;
      for (int t = 0; t < dk.n_terms; ++t) other_reader |= dk.term_t[t] == d1.out_t;
    }
    if (other_reader) continue;
    a1.stem2 = 1;
    a2.stem2 = 2;
  }
}

// 1x1 pairs (conv_pair.hip): the flags are the program's promise that the head's input and residual stay alive over the
// tail; whether the two ops ARE such a pair is checked here (anything else: the flags are ignored)
static void mark_pairs(rtpe_hrnet* h) {
  for (OpState& o : h->ops) o.pair = 0;
  for (size_t i = 0; i < h->ops.size(); ++i) {
    OpState& a1 = h->ops[i];
    if (!(a1.d.flags & RTPE_F_PAIR_HEAD) || i + 1 >= h->ops.size()) continue;
    const rtpe_op_desc &d1 = a1.d, &d2 = h->ops[i + 1].d;
    const int want1 = RTPE_F_RELU | RTPE_F_ROUND_CONV | RTPE_F_PAIR_HEAD, want2 = RTPE_F_RELU | RTPE_F_ROUND_CONV | RTPE_F_PAIR_TAIL;
    if (d1.kind != RTPE_OP_CONV || d2.kind != RTPE_OP_CONV || d1.flags != want1 || d2.flags != want2 || d1.ksize != 1 ||
        d2.ksize != 1 || d1.stride != 1 || d2.stride != 1 || d1.res_t < 0 || d2.res_t >= 0 || d2.in_t != d1.out_t ||
        d2.in_coff != d1.out_coff || d2.cin != d1.cout || !conv_pair_supports(d1.cin, d1.cout, d2.cout) ||
        h->tensors[d1.in_t].reserved == 4 || d1.reserved[2] > 0 || d2.reserved[2] > 0 || d2.out_t == d1.in_t ||
        d2.out_t == d1.res_t || d2.out_t == d1.out_t || d1.lane != d2.lane || d1.region != d2.region)
      continue;
    a1.pair = 1;
    h->ops[i + 1].pair = 2;
  }
}

// the skip projection of a pair's head (conv_pair.hip, PROJ): the one op p that writes the head's residual, a conv 1x1
// 64 -> 256 + bn of a tensor of the same map size, flagged RTPE_F_PAIR_PROJ (the program's promise that p's INPUT stays
// alive over the tail), whose output nobody else reads: the pair kernel computes it from p's input and p launches nothing
static void mark_projections(rtpe_hrnet* h) {
  for (OpState& o : h->ops) { o.proj_head = 0; o.proj_op = -1; }
  for (size_t i = 0; i < h->ops.size(); ++i) {
    if (h->ops[i].pair != 1) continue;
    const rtpe_op_desc& d1 = h->ops[i].d;
    int pi = -1, writers = 0;
    bool other_reader = d1.in_t == d1.res_t;
    for (size_t k = 0; k < h->ops.size(); ++k) {
      const rtpe_op_desc& dk = h->ops[k].d;
      if (dk.out_t == d1.res_t) { ++writers; pi = (int)k; }
      if (k == i) continue;
      if ((dk.kind != RTPE_OP_FUSE && dk.in_t == d1.res_t) || dk.res_t == d1.res_t) other_reader = true;
      for (int t = 0; t < dk.n_terms; ++t) other_reader |= dk.term_t[t] == d1.res_t;
    }
    if (writers != 1 || pi >= (int)i || other_reader) continue;
    OpState& op = h->ops[pi];
    const rtpe_op_desc& dp = op.d;
    const int round = d1.flags & RTPE_F_ROUND_CONV;
    if (dp.kind != RTPE_OP_CONV || op.n_geom != 1 || dp.ksize != 1 || dp.stride != 1 || dp.cin != 64 || dp.cout != 256 || dp.res_t >= 0 ||
        dp.n_terms != 0 || dp.flags != (round | RTPE_F_PAIR_PROJ) || dp.out_coff != 0 || d1.res_coff != 0 ||
        h->tensors[d1.res_t].channels != 256 || dp.reserved[1] > 1 || dp.reserved[2] > 0 || h->tensors[dp.in_t].reserved == 4 ||
        h->tensors[dp.in_t].ds_log2 != h->tensors[d1.in_t].ds_log2 || dp.in_t == d1.out_t || dp.in_t == h->ops[i + 1].d.out_t ||
        op.fuse || op.stem2 || op.pair)
      continue;
    // the pair reads p's input at the tail's launch: nobody may write it between p and the tail, and the tail's stream must be
    // behind whatever p's stream waited for (the head outside any region: behind the join; or on p's own lane)
    bool ok = d1.region == 0 || (d1.region == dp.region && d1.lane == dp.lane);
    for (size_t k = pi; k <= i + 1 && ok; ++k) ok = h->ops[k].d.out_t != dp.in_t;
    if (!ok) continue;
    op.proj_head = (int)i;
    h->ops[i].proj_op = pi;
  }
}

// neighbouring downsampling convs that read the same 48-channel tensor (the first convs of a fuse layer's chains from branch 0,
// pose_higher_hrnet.py:213-230: 48 -> 96 to branch 1, 48 -> 48 towards branches 2 and 3): one launch of conv48s2.hip reads the
// input once for all of them.  Static conditions here, the launch's own (sizes, layouts, option) in route_ops()
static void mark_s2_groups(rtpe_hrnet* h) {
  for (OpState& o : h->ops) o.s2g = 0;
  auto s2_static = [&](const OpState& o) {
    const rtpe_op_desc& d = o.d;
    return d.kind == RTPE_OP_CONV && d.ksize == 3 && d.stride == 2 && d.cin == 48 && (d.cout == 48 || d.cout == 96) && d.res_t < 0 &&
           !(d.flags & (RTPE_F_NO_NHWC | RTPE_F_F32 | RTPE_F_OUT_PREDS | RTPE_F_OUT_REFINED)) && o.n_geom == 1 && o.plan[0].esize == 2 &&
           o.plan[0].cout_pad == d.cout && d.reserved[2] <= 0;
  };
  static const int s2_groups = env_int("RTPE_S2_GROUPS", 1);
  for (size_t i = 0; s2_groups && i < h->ops.size(); ++i) {
    if (h->ops[i].s2g != 0 || !s2_static(h->ops[i])) continue;
    const rtpe_op_desc& d0 = h->ops[i].d;
    int n = 1, groups = d0.cout / 48;
    while (i + n < h->ops.size() && n < 3) {
      const OpState& on = h->ops[i + n];
      const rtpe_op_desc& dn = on.d;
      bool ok = s2_static(on) && dn.in_t == d0.in_t && dn.in_coff == d0.in_coff && dn.lane == d0.lane && dn.region == d0.region &&
                (dn.flags & RTPE_F_ROUND_CONV) == (d0.flags & RTPE_F_ROUND_CONV) && groups + dn.cout / 48 <= 4;
      for (int m = 0; m < n && ok; ++m) ok = h->ops[i + m].d.out_t != dn.out_t && dn.out_t != d0.in_t;
      if (!ok) break;
      groups += dn.cout / 48;
      ++n;
    }
    if (n < 2) continue;
    h->ops[i].s2g = n;
    for (int m = 1; m < n; ++m) h->ops[i + m].s2g = -1;
  }
}

// cross-lane dependencies inside parallel regions: the last writer of every tensor an op reads, when it ran on
// another lane of the same region (a region starts with a fork from and ends with a join into the caller's stream,
// so nothing outside it needs an event)
static int mark_lane_waits(rtpe_hrnet* h) {
  const int n_ops = (int)h->ops.size();
  h->needs_event.assign(n_ops, 0);
  h->wait_ops.assign(n_ops, std::vector<int>());
  std::vector<int> writer(h->tensors.size(), -1);
  std::vector<std::vector<int>> readers(h->tensors.size());     // ops that read a tensor since its last writer
  for (int i = 0; i < n_ops; ++i) {
    const rtpe_op_desc& d = h->ops[i].d;
    if (d.lane < 0 || d.lane > 3 || d.region < 0) { set_error("op %d: lane %d region %d", i, d.lane, d.region); return RTPE_E_INVALID; }
    if (d.region > 0) h->has_regions = true;
    if (d.region == 0 && d.lane != 0) { set_error("op %d: a lane outside a region", i); return RTPE_E_INVALID; }
    std::vector<int> reads;
    if (d.kind != RTPE_OP_FUSE && d.in_t >= 0) reads.push_back(d.in_t);
    if (d.res_t >= 0) reads.push_back(d.res_t);
    for (int t = 0; t < d.n_terms; ++t) reads.push_back(d.term_t[t]);
    if (d.out_t >= 0) reads.push_back(d.out_t);          // (a second writer of a shared buffer: ordered behind the first)
    for (int t : reads) {
      const int j = writer[t];
      if (j >= 0 && h->ops[j].d.region == d.region && d.region > 0 && h->ops[j].d.lane != d.lane) {
        h->needs_event[j] = 1;
        h->wait_ops[i].push_back(j);
      }
    }
    // write after read: a lane that overwrites a tensor (an in-place op, a shared slot written through `into=`) waits
    // for the ops of OTHER lanes that read the previous contents
    if (d.out_t >= 0) {
      for (int j : readers[d.out_t]) {
        if (j != i && h->ops[j].d.region == d.region && d.region > 0 && h->ops[j].d.lane != d.lane) {
          h->needs_event[j] = 1;
          h->wait_ops[i].push_back(j);
        }
      }
      readers[d.out_t].clear();
    }
    if (d.kind != RTPE_OP_FUSE && d.in_t >= 0) readers[d.in_t].push_back(i);
    if (d.res_t >= 0) readers[d.res_t].push_back(i);
    for (int t = 0; t < d.n_terms; ++t) readers[d.term_t[t]].push_back(i);
    if (d.out_t >= 0) writer[d.out_t] = i;
  }
  return RTPE_OK;
}

// tensors that may be kept plane-major (rtpe_hrnet::plane_ok)
static void mark_plane_major(rtpe_hrnet* h) {
  static const int plane_major = getenv("RTPE_PLANE_MAJOR") ? atoi(getenv("RTPE_PLANE_MAJOR")) : 1;
  h->plane_ok.assign(h->tensors.size(), 0);
  for (size_t t = 0; plane_major && t < h->tensors.size(); ++t) {
    const rtpe_tensor_desc& td = h->tensors[t];
    if (td.reserved == 4 || td.channels < 96 || td.channels % 48 != 0) continue;
    bool ok = true, touched = false;
    for (const OpState& o : h->ops) {
      const rtpe_op_desc& d = o.d;
      bool uses = d.in_t == (int)t || d.out_t == (int)t || d.res_t == (int)t;
      for (int k = 0; k < d.n_terms; ++k) uses |= d.term_t[k] == (int)t;
      if (!uses) continue;
      touched = true;
      const int clean = RTPE_F_RELU | RTPE_F_ROUND_CONV;
      if (d.kind != RTPE_OP_CONV || o.n_geom != 1 || d.n_terms != 0 || (d.flags & ~clean) || d.ksize != 3 ||
          d.stride != 1 || !conv_stream_supports(o.plan[0]) || o.plan[0].mt != 3 || d.cout % 48 != 0 ||
          d.in_coff != 0 || d.out_coff != 0 || (d.res_t >= 0 && d.res_coff != 0) || d.reserved[2] != 0 ||
          d.cin != h->tensors[d.in_t].channels || d.cout != h->tensors[d.out_t].channels ||
          (d.res_t >= 0 && h->tensors[d.res_t].channels != d.cout)) {
        ok = false;
        break;
      }
    }
    h->plane_ok[t] = ok && touched;
  }
}

// pack on the host, one upload
static int pack_and_upload(rtpe_hrnet* h, const void* weights) {
  const char* wb = reinterpret_cast<const char*>(weights);
  const int n_ops = (int)h->ops.size();
  const size_t off = h->arena_bytes;
  std::vector<char> host(off, 0);
  for (int i = 0; i < n_ops; ++i) {
    OpState& o = h->ops[i];
    const rtpe_op_desc& d = o.d;
    if (d.kind == RTPE_OP_CONV || d.kind == RTPE_OP_DECONV) {
      for (int k = 0; k < o.n_geom; ++k)
        conv_pack_weights(o.geom[k], o.plan[k], wb + d.w_off, host.data() + o.w_dev_off[k]);
      float* ab = reinterpret_cast<float*>(host.data() + o.ab_dev_off);
      const float* src = reinterpret_cast<const float*>(wb + d.ab_off);
      const int cp = o.plan[0].cout_pad;
      for (int c = 0; c < d.cout; ++c) { ab[c] = src[c]; ab[cp + c] = src[d.cout + c]; }
    } else if (d.kind == RTPE_OP_STEM) {
      const int es = (d.flags & RTPE_F_F32) ? 4 : 2;                 // (64,3,3,3) in the program's precision
      const char* w = wb + d.w_off;
      char* p = host.data() + o.w_dev_off[0];
      for (int co = 0; co < 64; ++co)
        for (int c = 0; c < 3; ++c)
          for (int ky = 0; ky < 3; ++ky)
            for (int kx = 0; kx < 3; ++kx)
              memcpy(p + (size_t)(((ky * 3 + kx) * 3 + c) * 64 + co) * es,
                     w + (size_t)(((co * 3 + c) * 3 + ky) * 3 + kx) * es, es);
      memcpy(host.data() + o.ab_dev_off, wb + d.ab_off, 2 * 64 * sizeof(float));
    } else if (d.kind == RTPE_OP_SE) {
      memcpy(host.data() + o.w_dev_off[0], wb + d.w_off, ((size_t)d.cout * d.cin * 2 + d.cout + d.cin) * 4);
    }
  }
  hipError_t e = hipMalloc(reinterpret_cast<void**>(&h->arena), off ? off : 256);
  if (e != hipSuccess) { h->arena = nullptr; return hip_fail(e, "hipMalloc(arena)", __FILE__, __LINE__); }
  e = hipMemcpy(h->arena, host.data(), off, hipMemcpyHostToDevice);
  if (e != hipSuccess) return hip_fail(e, "hipMemcpy(arena)", __FILE__, __LINE__);     // (the caller frees the arena)
  return RTPE_OK;
}

extern "C" int rtpe_hrnet_create(const rtpe_op_desc* ops, int32_t n_ops,
                                 const rtpe_tensor_desc* tensors, int32_t n_tensors,
                                 const void* weights, size_t weights_bytes, int32_t device,
                                 rtpe_hrnet** out) {
  RTPE_REQUIRE(ops && tensors && weights && out && n_ops > 0 && n_tensors > 0, "hrnet_create: null argument");
  DeviceGuard guard(device);               // the caller's current device is restored on return
  RTPE_HIP_CHECK(guard.err);
  rtpe_hrnet* h = new rtpe_hrnet();
  h->device = device;
  h->tensors.assign(tensors, tensors + n_tensors);
  h->n_slots = 0;
  for (auto& t : h->tensors) h->n_slots = t.slot + 1 > h->n_slots ? t.slot + 1 : h->n_slots;
  h->n_preds = h->n_refined = 0;
  h->arena = nullptr;
  int rc = plan_ops(h, ops, n_ops, weights_bytes);
  if (rc == RTPE_OK) {
    mark_blocks(h);
    mark_stems(h);
    mark_pairs(h);
    mark_projections(h);
    mark_s2_groups(h);
    rc = mark_lane_waits(h);
  }
  if (rc == RTPE_OK) {
    mark_plane_major(h);
    rc = pack_and_upload(h, weights);
  }
  if (rc != RTPE_OK) {                     // (the message of the pass that failed stands)
    if (h->arena) hipFree(h->arena);
    delete h;
    return rc;
  }
  *out = h;
  return RTPE_OK;
}

extern "C" int rtpe_hrnet_destroy(rtpe_hrnet* h) {
  if (!h) return RTPE_OK;
  DeviceGuard guard(h->device);
  for (auto& kv : h->records)
    for (auto& e : kv.second.ev) hipEventDestroy(e);
  for (auto& e : h->op_event) if (e) hipEventDestroy(e);
  if (h->fork_event) hipEventDestroy(h->fork_event);
  for (int l = 1; l < 4; ++l) if (h->lane_stream[l]) hipStreamDestroy(h->lane_stream[l]);
  if (h->arena) hipFree(h->arena);
  delete h;
  return RTPE_OK;
}

static void slot_layout(const rtpe_hrnet* h, int N, int H, int W, std::vector<size_t>* offs, size_t* total) {
  std::vector<size_t> sz(h->n_slots, 0);
  for (const auto& t : h->tensors) {
    const size_t px = t.ds_log2 < 0 ? 1 : (size_t)extent(H, t.ds_log2) * extent(W, t.ds_log2);
    const size_t b = (size_t)N * px * t.channels * (t.reserved == 4 ? 4 : 2);
    if (b > sz[t.slot]) sz[t.slot] = b;
  }
  offs->resize(h->n_slots);
  size_t o = 0;
  for (int s = 0; s < h->n_slots; ++s) { (*offs)[s] = o; o += align_up(sz[s], 256); }
  *total = o;
}

// The shapes a handle takes, checked before anything is sized or launched.  Multiples of 32: every program.  Ragged shapes (a side
// that is no multiple of 32): programs with the any_size property whose ops all have a general path - a transposed conv doubles a
// map that the extent rule does not double, and a fused BasicBlock pair or a stride-2 group has no launch of its own to fall
// back to in the records of a forward.  The nearest-to-size sampler of the fuse ops has one row of workgroups per output row.
// A mixed-size batch (`mixed`, rtpe_hip_mixed.h) is held to the rules of a ragged shape whatever its canvas size, and its ops
// to those that mask by the extent table: no tensor below 1/32 read by a conv, a resize, a fuse sum or an SE mean.  A program
// with a second input goes through rtpe_hrnet_forward_mixed_aux (rtpe_hip_mixed_aux.h), which brings it (`aux_ok`); the entry
// without one refuses it here.
static int check_shape(const rtpe_hrnet* h, int N, int H, int W, const char* who, bool mixed = false, bool aux_ok = false) {
  RTPE_REQUIRE(N > 0 && H >= 32 && W >= 32, "%s: N=%d H=%d W=%d", who, N, H, W);
  if (mixed) {
    RTPE_REQUIRE(h->any_size, "%s: a mixed-size batch needs a program with the any_size property (the students'); this program "
                 "takes one size per batch, multiples of 32", who);
    for (size_t i = 0; i < h->ops.size(); ++i) {
      const rtpe_op_desc& d = h->ops[i].d;
      const bool aux_op = d.kind == RTPE_OP_AUX_PACK || d.kind == RTPE_OP_RESIZE || d.kind == RTPE_OP_GATE_MUL;
      RTPE_REQUIRE(aux_ok || !aux_op,
                   "%s: op %zu: a program with a second input (aux pack, resize, gate_mul) takes a mixed-size batch through "
                   "rtpe_hrnet_forward_mixed_aux only", who, i);
      RTPE_REQUIRE(!aux_op || (d.flags & RTPE_F_F32),
                   "%s: op %zu: the fp16 forms of the second-input ops (aux pack, resize, gate_mul) have no masked form yet: a half "
                   "body with a second input takes one size per batch", who, i);
      int top = -1;                                     // the deepest level whose row of the table this op reads
      if (d.kind == RTPE_OP_RESIZE) top = h->tensors[d.in_t].ds_log2 > h->tensors[d.out_t].ds_log2 ? h->tensors[d.in_t].ds_log2 : h->tensors[d.out_t].ds_log2;
      if (d.kind == RTPE_OP_CONV) top = h->tensors[d.in_t].ds_log2 + (d.stride == 2 ? 1 : 0);
      if (d.kind == RTPE_OP_STEM) top = 1;
      if (d.kind == RTPE_OP_AVGPOOL || d.kind == RTPE_OP_SE) top = h->tensors[d.in_t].ds_log2;
      if (d.kind == RTPE_OP_FUSE) {
        top = h->tensors[d.out_t].ds_log2;
        for (int t = 0; t < d.n_terms; ++t) top = h->tensors[d.term_t[t]].ds_log2 > top ? h->tensors[d.term_t[t]].ds_log2 : top;
      }
      RTPE_REQUIRE(top < RTPE_MIXED_LEVELS, "%s: op %zu works at 1 / 2^%d, the extent table ends at 1 / 2^%d", who, i, top,
                   RTPE_MIXED_LEVELS - 1);
    }
  }
  if (!ragged(H, W) && !mixed) return RTPE_OK;
  RTPE_REQUIRE(h->any_size, "%s: N=%d H=%d W=%d: H and W must be multiples of 32 for this program (its branches at 1/4 .. 1/32 "
               "are fused by factor-2 resampling; only programs with the any_size property take other sizes)", who, N, H, W);
  for (size_t i = 0; i < h->ops.size(); ++i) {
    const OpState& o = h->ops[i];
    RTPE_REQUIRE(o.d.kind != RTPE_OP_DECONV && o.fuse == 0 && o.s2g == 0,
                 "%s: op %zu (%s) cannot take a map of %d x %d input pixels (sides that are no multiples of 32)", who, i,
                 o.d.kind == RTPE_OP_DECONV ? "transposed conv" : o.fuse ? "fused BasicBlock pair" : "grouped stride-2 conv", H, W);
    if (o.d.kind == RTPE_OP_FUSE) {
      const rtpe_tensor_desc& to = h->tensors[o.d.out_t];
      RTPE_REQUIRE(fuse_nearest_supports(N, extent(H, to.ds_log2), extent(W, to.ds_log2), o.d.cout, (o.d.flags & RTPE_F_F32) ? 1 : 0),
                   "%s: op %zu: a fuse sum of %d x %d x %d is too large for the nearest-to-size sampler", who, i, N,
                   extent(H, to.ds_log2), extent(W, to.ds_log2));
    }
  }
  return RTPE_OK;
}

extern "C" int rtpe_hrnet_workspace_bytes(const rtpe_hrnet* h, int32_t N, int32_t H, int32_t W, size_t* bytes) {
  RTPE_REQUIRE(h && bytes && N > 0 && H > 0 && W > 0 && (h->any_size || !ragged(H, W)),
               "workspace_bytes: N=%d H=%d W=%d (H, W must be multiples of 32)", N, H, W);
  std::vector<size_t> offs;
  slot_layout(h, N, H, W, &offs, bytes);
  return RTPE_OK;
}

// plane-major tensors of one run: the candidates all of whose ops run on the streaming kernel with the launch
// shapes in force (tiny maps fall back to the generic kernel, which only knows NHWC)
static std::vector<char> plane_tensors(const rtpe_hrnet* h, int N, int H, int W, const std::vector<ConvTile>* tuned, bool rag) {
  if (rag) return std::vector<char>(h->plane_ok.size(), 0);   // (the streaming kernel, which alone knows the layout, is not used)
  std::vector<char> plane = h->plane_ok;
  for (size_t i = 0; i < h->ops.size(); ++i) {
    const OpState& o = h->ops[i];
    const rtpe_op_desc& d = o.d;
    if (d.kind != RTPE_OP_CONV || o.n_geom != 1) continue;
    if (!(plane[d.in_t] || plane[d.out_t] || (d.res_t >= 0 && plane[d.res_t]))) continue;
    const rtpe_tensor_desc& ti = h->tensors[d.in_t];
    const ConvTile t = (tuned && (*tuned)[i * 4].nt) ? (*tuned)[i * 4]
                                                      : conv_make_tile(o.plan[0], N, extent(H, ti.ds_log2), extent(W, ti.ds_log2));
    if (t.kind != 2) {
      plane[d.in_t] = plane[d.out_t] = 0;
      if (d.res_t >= 0) plane[d.res_t] = 0;
    }
  }
  return plane;
}

// the kernel-selecting options, read once per forward
struct RouteOpts {
  int fused_stem = get_option(kOptFusedStem), pair_1x1 = get_option(kOptPair1x1), pair_proj = get_option(kOptPairProj),
      conv64 = get_option(kOptConv64), head_direct = get_option(kOptHeadDirect), deconv48 = get_option(kOptDeconv48),
      conv48s2 = get_option(kOptConv48s2);
};

// what a forward binds: shape, buffers, tuned launch shapes, plane-major tensors.  (rtpe_hrnet_op_tile binds nominal buffers:
// the routes depend on their being there and on their alignment only, nothing is dereferenced before a launch)
struct Fwd {
  const rtpe_hrnet* h;
  int N, H, W;
  char* base;
  void *preds, *refined;
  int out_dtype;
  std::vector<size_t> offs;
  size_t ws_need;
  const std::vector<ConvTile>* tuned = nullptr;
  std::vector<char> plane;
  bool rag;                 // a ragged shape: general paths, default launch shapes (nothing is tuned at such a shape)
  const int32_t* ext;       // a mixed-size batch (always `rag`): the extent table on the device, else nullptr
  const int32_t* level(int ds) const { return ext + (size_t)ds * 2 * N; }     // (h, w) of every image at 1 / 2^ds
  Fwd(const rtpe_hrnet* h_, int N_, int H_, int W_, void* ws, void* preds_, void* refined_, int out_dtype_, const int32_t* ext_ = nullptr)
      : h(h_), N(N_), H(H_), W(W_), base(reinterpret_cast<char*>(ws)), preds(preds_), refined(refined_), out_dtype(out_dtype_),
        rag(ragged(H_, W_) || ext_ != nullptr), ext(ext_) {
    slot_layout(h, N, H, W, &offs, &ws_need);
    auto it = h->tuned.find(std::make_tuple(N, H, W));
    if (it != h->tuned.end() && !rag) tuned = &it->second;
    plane = plane_tensors(h, N, H, W, tuned, rag);
  }
  size_t esz(int t) const { return h->tensors[t].reserved == 4 ? 4 : 2; }
  _Float16* tptr(int t, int coff) const {      // element type per tensor (fp16 or fp32): byte arithmetic
    return reinterpret_cast<_Float16*>(base + offs[h->tensors[t].slot] + (size_t)coff * esz(t));
  }
  ConvTile tile(size_t i, int k, int H_pos, int W_pos) const {   // tuned, else the default; ragged: the kernel that takes every shape
    if (rag) return conv_make_tile(h->ops[i].plan[k], N, H_pos, W_pos, /*allow_direct=*/false, /*allow_conv64=*/false, /*allow_stream=*/false);
    return tuned && (*tuned)[i * 4 + k].nt ? (*tuned)[i * 4 + k] : conv_make_tile(h->ops[i].plan[k], N, H_pos, W_pos);
  }
};

extern "C" int rtpe_hrnet_plane_major_tensors(const rtpe_hrnet* h, int32_t N, int32_t H, int32_t W, int32_t* count) {
  RTPE_REQUIRE(h != nullptr && count != nullptr, "plane_major_tensors: null argument");
  {
    const int rc = check_shape(h, N, H, W, "plane_major_tensors");
    if (rc != RTPE_OK) return rc;
  }
  const Fwd f(h, N, H, W, nullptr, nullptr, nullptr, RTPE_DTYPE_F32);
  *count = 0;
  for (char c : f.plane) *count += c;
  return RTPE_OK;
}

// the grid of output positions of conv op i per side: the input map of a transposed conv (one launch class per sub-pixel), else the
// extent of the output, one stride-2 step below the input's (= the input's extent / stride for multiples of 32; ceil otherwise)
static int conv_pos(const rtpe_hrnet* h, const rtpe_op_desc& d, int n) {
  const int ds = h->tensors[d.in_t].ds_log2;
  return extent(n, d.kind == RTPE_OP_DECONV || d.stride != 2 ? ds : ds + 1);
}

// argument block of parity class k of conv op i: pointers, sizes and flags (the launch shape's half is conv_fill_args')
static ConvArgs conv_op_args(const Fwd& f, size_t i, int k) {
  const rtpe_hrnet* h = f.h;
  const OpState& o = h->ops[i];
  const rtpe_op_desc& d = o.d;
  const rtpe_tensor_desc& ti = h->tensors[d.in_t];
  const int N = f.N, Hi = extent(f.H, ti.ds_log2), Wi = extent(f.W, ti.ds_log2);
  const bool dc = d.kind == RTPE_OP_DECONV;
  const int Ho = dc ? Hi * 2 : conv_pos(h, d, f.H), Wo = dc ? Wi * 2 : conv_pos(h, d, f.W);
  ConvArgs a;
  memset(&a, 0, sizeof(a));
  a.x = f.tptr(d.in_t, d.in_coff);
  a.in_ld = ti.channels;
  if (f.plane[d.in_t]) { a.in_ld = 48; a.in_cs = (long long)N * Hi * Wi * 48; }
  a.x_bytes = ((size_t)N * Hi * Wi * ti.channels - (size_t)d.in_coff) * f.esz(d.in_t);
  a.w = reinterpret_cast<const _Float16*>(h->arena + o.w_dev_off[k]);
  a.alpha = reinterpret_cast<const float*>(h->arena + o.ab_dev_off);
  a.beta = a.alpha + o.plan[0].cout_pad;
  if (d.res_t >= 0) {
    a.res = f.tptr(d.res_t, d.res_coff);
    a.res_ld = h->tensors[d.res_t].channels;
    if (f.plane[d.res_t]) { a.res_ld = 48; a.res_cs = (long long)N * Ho * Wo * 48; }
  }
  if (!(d.flags & RTPE_F_NO_NHWC)) {
    a.y = f.tptr(d.out_t, d.out_coff);
    a.out_ld = h->tensors[d.out_t].channels;
    if (f.plane[d.out_t]) { a.out_ld = 48; a.out_cs = (long long)N * Ho * Wo * 48; }
    // zero-padded channels up to the allocated row are written too (they
    // are exact zeros: zero weights, zero affine) so that a consumer that
    // reads the padded view sees finite data
    int cs = o.plan[0].cout_pad;
    const int room = h->tensors[d.out_t].channels - d.out_coff;
    a.cout_store = cs < room ? cs : room;
    if (d.reserved[2] > 0 && d.reserved[2] < a.cout_store) a.cout_store = d.reserved[2];
  }
  if (d.flags & RTPE_F_OUT_PREDS) { a.y_nchw = f.preds; a.nchw_channels = d.cout; }
  if (d.flags & RTPE_F_OUT_REFINED) { a.y_nchw = f.refined; a.nchw_channels = d.cout; }
  a.nchw_f32 = f.out_dtype == RTPE_DTYPE_F32;
  a.N = N; a.H_in = Hi; a.W_in = Wi;
  a.H_full = Ho; a.W_full = Wo;
  if (dc) {
    a.H_pos = Hi; a.W_pos = Wi; a.o_mul = 2; a.oy_add = k >> 1; a.ox_add = k & 1;
  } else {
    a.H_pos = Ho; a.W_pos = Wo; a.o_mul = 1;
  }
  a.relu = (d.flags & RTPE_F_RELU) ? 1 : 0;
  a.round_conv = (d.flags & RTPE_F_ROUND_CONV) ? 1 : 0;
  if (f.ext != nullptr) {     // (no transposed conv in a mixed-size batch: check_shape) a stride-2 conv writes the next level
    a.mixed = 1;
    a.ext_in = f.level(ti.ds_log2);
    a.ext_out = f.level(ti.ds_log2 + (d.stride == 2 ? 1 : 0));
  }
  return a;
}

static ConvArgs conv_op_args(const Fwd& f, size_t i, int k, const ConvTile& t) {
  ConvArgs a = conv_op_args(f, i, k);
  conv_fill_args(f.h->ops[i].geom[k], f.h->ops[i].plan[k], t, &a);
  return a;
}

// the direct 1x1 kernel, the 1x1 pair and the persistent kernels address their input through one 2-GiB buffer window and write
// plain NHWC rows: a larger view (batch >= 164 at 640 x 640 for the 256 -> 64 conv) or another output form takes the
// one-workgroup-per-tile kernel, whose staging falls back per image
static bool conv_direct_ok(const ConvArgs& a) {
  return a.x_bytes < 0x80000000ull && a.y != nullptr && a.y_nchw == nullptr && a.o_mul == 1;
}

// The per-conv decision (the executor's ops and the single-layer entries).  First the rules that override a launch shape:
// kind 4 needs direct_ok; kind 5 (conv64.hip) also takes no residual and no plane-major tensor (plane_io: the input or the
// NHWC output is one) - also when a tuned or imported shape says kind 5 but option "conv64" has been switched off since
static void conv_fix_tile(const RouteOpts& opt, const ConvPlan& p, const ConvArgs& a, bool plane_io, ConvTile* t) {
  const bool direct_ok = conv_direct_ok(a);
  if (t->kind == 4 && !direct_ok) *t = conv_make_tile(p, a.N, a.H_pos, a.W_pos, /*allow_direct=*/false);
  if (t->kind == 5 && !(direct_ok && a.res == nullptr && !plane_io && opt.conv64 != 0))
    *t = conv_make_tile(p, a.N, a.H_pos, a.W_pos, true, /*allow_conv64=*/false);
}

// ... then the kernel, for arguments filled on that shape: the heads (1x1, 48 input channels, fp32 NCHW out) and the
// downsampling convs from 48 input channels have kernels of their own, whatever launch shape was chosen or tuned for the layer
static int conv_pick(const RouteOpts& opt, const ConvPlan& p, const ConvTile& t, const ConvArgs& a, bool plane_io) {
  if (opt.head_direct != 0 && conv_head_supports(p, a)) return kRouteHead;
  if (opt.conv48s2 != 0 && !plane_io && conv48s2_supports(p, a)) return kRouteS2;
  return t.kind == 2 ? kRouteStream : t.kind == 4 ? kRouteDirect : t.kind == 5 ? kRouteConv64 : kRouteTile;
}

// the 4 sub-pixel classes of a transposed conv run as ONE grid (conv_mfma.hip) on class 0's launch shape when that shape is a
// one-workgroup-per-tile one and the plans of all classes agree (they differ in the tap offsets and the packed weights only;
// RTPE_DECONV_MERGE=0: four launches)
static bool deconv_merges(const ConvPlan* p, const ConvTile& tile0) {
  static const int merge_deconv = env_int("RTPE_DECONV_MERGE", 1);
  bool merge = merge_deconv && tile0.kind == 0;
  for (int k = 1; k < 4 && merge; ++k)
    merge = p[k].mt == p[0].mt && p[k].cc == p[0].cc && p[k].kc == p[0].kc && p[k].n_cchunks == p[0].n_cchunks &&
            p[k].n_cb == p[0].n_cb && p[k].pstride == p[0].pstride && p[k].tapw == p[0].tapw;
  return merge;
}

// class k's weights and offsets go into the argument block of class 0
static void deconv_merge_class(ConvArgs* merged, const ConvArgs& a, int k) {
  if (k == 0) { *merged = a; merged->n_cls = 4; }
  merged->w_c[k] = a.w;
  merged->lo_yc[k] = a.lo_y; merged->lo_xc[k] = a.lo_x;
  merged->oy_c[k] = a.oy_add; merged->ox_c[k] = a.ox_add;
}

static ConvArgs deconv_merged_args(const Fwd& f, size_t i, const ConvTile& tile0) {
  ConvArgs merged;
  for (int k = 0; k < 4; ++k) deconv_merge_class(&merged, conv_op_args(f, i, k, tile0), k);
  return merged;
}

// the four classes on one persistent kernel that shares their halo tiles (deconv48.hip, option "deconv48")
static int deconv_pick(const RouteOpts& opt, const ConvPlan& p0, const ConvArgs& merged) {
  return opt.deconv48 != 0 && deconv48_supports(p0, merged) ? kRouteDeconv48 : kRouteDeconvMerged;
}

static int launch_conv(int how, const ConvPlan& p, const ConvTile& t, const ConvArgs& a, hipStream_t s) {
  switch (how) {
    case kRouteHead: return conv_head_launch(p, a, s);
    case kRouteS2: return conv48s2_launch(p, a, s);
    case kRouteDeconv48: return deconv48_launch(p, a, s);
    default: return conv_launch(p, t, a, s);
  }
}

// args[i]: the argument block the pass built for conv op i (class 0 on its launch shape; a merged transposed conv: all four
// classes) - what the launch that computes op i hands to the kernel.  Both outputs are indexed by op; a stride-2 group hands
// args[i .. i + n) to its launch as one array
static int route_ops(const Fwd& f, std::vector<Route>* routes, std::vector<ConvArgs>* args) {
  const rtpe_hrnet* h = f.h;
  const RouteOpts opt;
  routes->assign(h->ops.size(), Route());
  args->assign(h->ops.size(), ConvArgs());
  for (size_t i = 0; i < h->ops.size(); ++i) {
    Route& r = (*routes)[i];
    const OpState& o = h->ops[i];
    const rtpe_op_desc& d = o.d;
    auto absorb = [&](size_t j) { (*routes)[j].how = kRouteDoneBy; (*routes)[j].by = (int)i; };
    if (r.how == kRouteDoneBy) continue;
    if (d.kind == RTPE_OP_STEM) {
      const int fused = !f.rag && stem_fused_supports(f.H, f.W) ? opt.fused_stem : 0;
      r.how = fused == 1 && o.stem2 == 1 ? kRouteStemFused : fused == 2 && !(d.flags & RTPE_F_F32) ? kRouteStemConv1 : kRouteStemPlain;
      if (r.how == kRouteStemFused) absorb(i + 1);
      continue;
    }
    if (o.n_geom == 0) continue;
    if (d.flags & (RTPE_F_OUT_PREDS | RTPE_F_OUT_REFINED))
      RTPE_REQUIRE(((d.flags & RTPE_F_OUT_REFINED) ? f.refined : f.preds) != nullptr, "forward: output pointer missing");
    const rtpe_tensor_desc& ti = h->tensors[d.in_t];
    const int Hi = extent(f.H, ti.ds_log2), Wi = extent(f.W, ti.ds_log2);
    const bool dc = d.kind == RTPE_OP_DECONV;
    // a flagged BasicBlock pair runs as one kernel from 6 x 16 maps up; a smaller map runs both convs on their own.  (A fused
    // kernel for the 96-channel branch was built and measured in round 5 - slower than the two streaming launches:
    // profiles/r05_block96_ablation.txt, tools/experiments/conv_block96.hip.)
    if (o.fuse == 1 && conv_block_supports(d.cin, d.cout, Hi, Wi)) {     // (never at a ragged shape: check_shape)
      r.how = kRouteBlock;
      absorb(i + 1);
      continue;
    }
    for (int k = 0; k < o.n_geom; ++k) r.tile[k] = f.tile(i, k, conv_pos(h, d, f.H), conv_pos(h, d, f.W));
    if (f.rag) {       // every conv on the one-workgroup-per-tile kernel, which masks its reads and stores at every edge
      RTPE_REQUIRE(f.ext == nullptr || conv_has_mixed_variant(o.plan[0].mt, r.tile[0].nt, r.tile[0].waves),
                   "forward: op %zu: no mixed-size kernel variant mt=%d nt=%d waves=%d", i, o.plan[0].mt, r.tile[0].nt, r.tile[0].waves);
      (*args)[i] = conv_op_args(f, i, 0, r.tile[0]);
      r.how = kRouteTile;
      continue;
    }
    if (dc && deconv_merges(o.plan, r.tile[0])) {
      (*args)[i] = deconv_merged_args(f, i, r.tile[0]);
      r.how = deconv_pick(opt, o.plan[0], (*args)[i]);
      continue;
    }
    // the first downsampling convs of a fuse layer's chains from one branch (OpState::s2g): one launch, the input read once
    if (o.s2g > 1 && opt.conv48s2 != 0) {
      bool ok = true;
      for (int m = 0; m < o.s2g && ok; ++m) {
        const OpState& om = h->ops[i + m];
        Route& rm = (*routes)[i + m];
        if (m > 0) rm.tile[0] = f.tile(i + m, 0, Hi / 2, Wi / 2);
        (*args)[i + m] = conv_op_args(f, i + m, 0, rm.tile[0]);
        ok = !f.plane[om.d.in_t] && !f.plane[om.d.out_t] && conv48s2_supports(om.plan[0], (*args)[i + m]);
      }
      if (ok) {
        r.how = kRouteS2Group;
        r.by = o.s2g;
        for (int m = 1; m < o.s2g; ++m) absorb(i + m);
        continue;
      }
    }
    const bool plane_io = f.plane[d.in_t] || (!(d.flags & RTPE_F_NO_NHWC) && f.plane[d.out_t]);
    ConvArgs& a = (*args)[i];
    a = conv_op_args(f, i, 0);
    for (int k = 0; k < o.n_geom; ++k) conv_fix_tile(opt, o.plan[k], k ? conv_op_args(f, i, k) : a, plane_io, &r.tile[k]);
    conv_fill_args(o.geom[0], o.plan[0], r.tile[0], &a);
    if (r.how == kRoutePairTail) continue;               // marked at its head
    r.how = conv_pick(opt, o.plan[0], r.tile[0], a, plane_io);       // (the classes of an unmerged transposed conv: o_mul = 2, neither a head nor a stride-2 conv)
    if (r.how == kRouteHead || r.how == kRouteS2 || opt.pair_1x1 == 0 || !conv_direct_ok(a)) continue;
    // a 1x1 pair is launched at its tail.  Its flagged skip projection (OpState::proj_head) is computed there too, option
    // "pair_proj", when both input views lie inside the window (the head's other conditions follow from the flags that made it one)
    if (o.proj_head > 0 && opt.pair_proj != 0 && conv_direct_ok(conv_op_args(f, o.proj_head, 0))) {
      r.how = kRoutePairProj;
      r.by = o.proj_head + 1;
    } else if (o.pair == 1) {
      r.how = kRoutePairHead;
      r.by = (int)i + 1;
      (*routes)[i + 1].how = kRoutePairTail;
      (*routes)[i + 1].by = (int)i;
    }
  }
  for (size_t i = 0; i < h->ops.size(); ++i)              // a folded projection is computed nowhere else
    RTPE_REQUIRE((*routes)[i].how != kRoutePairProj || (*routes)[h->ops[i].proj_head].how == kRoutePairHead,
                 "forward: op %d is no 1x1 pair head at this shape, its projection was folded", h->ops[i].proj_head);
  return RTPE_OK;
}

// rtpe_hrnet_op_tile's out8 for a route
static void route_label(const rtpe_hrnet* h, const std::vector<Route>& routes, size_t i, int32_t* out8) {
  const Route& r = routes[i];
  const OpState& o = h->ops[i];
  const ConvTile& t = r.tile[0];
  const int by = r.how == kRouteDoneBy ? routes[r.by].how : kRouteNone;
  auto set = [&](int mt, int nt, int waves, int th, int tw, int cc, int n_cb, int v) {
    const int32_t l[8] = {mt, nt, waves, th, tw, cc, n_cb, v};
    memcpy(out8, l, sizeof(l));
  };
  memset(out8, 0, 8 * sizeof(int32_t));
  if (r.how == kRouteStemFused || by == kRouteStemFused) {            // stem_fused.hip: 8 x 16 tiles, 8 waves
    set(4, 4, 8, 8, 16, 64, 1, by ? -600002 : -600001);
  } else if (r.how == kRouteBlock || by == kRouteBlock) {             // conv_block.hip: 6x32 tiles, 5 + 3 pixel tiles per wave
    set(3, by ? 3 : 5, 4, 6, 32, 48, 1, by ? -900002 : -900001);
  } else if (r.how == kRouteS2 || r.how == kRouteS2Group || by == kRouteS2Group) {
    // conv48s2.hip: 8 x 8 output tiles, a wave = one group of 48 output channels.  -200001: a launch of its own; -20000n
    // (n = 2, 3): first of n convs from one input in ONE launch; -200009: one of the others
    const int gw = o.d.cout == 48 ? 1 : o.d.cout == 96 ? 2 : 4;
    set(3, 2, 4, 8, 8, 48, o.d.cout / (48 * gw), by ? -200009 : r.how == kRouteS2Group ? -(200000 + r.by) : -200001);
  } else if (r.how == kRouteHead) {                                   // conv_direct.hip's head kernel: 32 pixels per wave step
    set(o.plan[0].mt, 2, 4, 1, 32, 48, 1, -400001);
  } else if (r.how == kRouteDeconv48) {                               // deconv48.hip: 8 x 16 input positions per tile, wave k = class k
    set(3, 2, 4, 8, 16, 48, 1, -300001);
  } else if (r.how == kRoutePairProj) {                               // conv_pair.hip: 16-pixel tiles per wave, 8 waves; no launch of its own
    set(0, 1, 8, 1, 16, 64, 1, -800003);
  } else if (r.how == kRoutePairHead || r.how == kRoutePairTail) {
    const bool head = r.how == kRoutePairHead;
    set(head ? 16 : 4, 1, 8, 1, 16, head ? 64 : 256, 1, head ? -800001 : -800002);
  } else if (o.n_geom > 0) {                                          // conv_launch on the launch shape (of class 0)
    set(t.kind == 0 && t.mrun ? t.mrun : o.plan[0].mt, t.nt, t.waves, t.th, t.tw, o.plan[0].cc, o.plan[0].n_cb,
        t.kind == 2 ? -(t.grid + 100000 * t.n_bufs) : t.kind == 4 ? -(700000 + t.grid) : t.kind == 5 ? -(500000 + t.grid) : (int32_t)t.lds_bytes);
  }
}

// Per-op HIP events.  An op absorbed by the fused launch of its predecessor has none (its time is 0), and a fused
// block that is followed at once by another one has none either: a marker packet between two kernels costs ~3 us
// of stream time (3-4 % of this kernel), so a run of consecutive fused blocks is bracketed as a whole and its
// blocks share the interval equally - the per-launch time then agrees with the kernel trace.
static bool block_head(const std::vector<Route>& r, size_t i) { return i < r.size() && r[i].how == kRouteBlock; }
static bool block_tail(const std::vector<Route>& r, size_t i) { return i > 0 && block_head(r, i - 1); }

static bool op_has_event(const std::vector<Route>& r, size_t i) {
  return !block_tail(r, i) && !(block_head(r, i) && block_head(r, i + 2));
}

static int read_op_times(const std::vector<Route>& r, const std::vector<hipEvent_t>& ev, float* op_ms) {
  for (size_t i = 0; i < r.size(); ++i) {
    if (block_tail(r, i)) { op_ms[i] = 0.f; continue; }
    size_t first = i, last = i;
    if (block_head(r, i)) {
      while (first >= 2 && block_head(r, first - 2)) first -= 2;
      while (block_head(r, last + 2)) last += 2;
    }
    // the interval starts at the event of the op before `first` (a run never starts behind an absorbed op; any
    // other op that follows an absorbed one starts at the event of that block's head)
    const size_t b0 = first > 0 && block_tail(r, first - 1) ? first - 1 : first;
    float ms;
    RTPE_HIP_CHECK(hipEventElapsedTime(&ms, ev[b0], ev[last + 1]));
    op_ms[i] = ms / (float)((last - first) / 2 + 1);
  }
  return RTPE_OK;
}

// ---- one forward: run() and its parts ------------------------------------------------------------------------------------
namespace {   // (the classes below are the executor's own: nothing of them is exported)

// What a forward is called with.  The entries fill the bound part through fwd_call() and set the rest where they are about it
struct FwdCall {
  const void* x = nullptr;                       // the images, NCHW
  int x_dtype = 0, N = 0, H = 0, W = 0;
  void *preds = nullptr, *refined = nullptr;     // the two NCHW outputs
  int out_dtype = 0;
  void* ws = nullptr;
  size_t ws_bytes = 0;
  hipStream_t stream = nullptr;                  // the caller's stream
  const void* aux = nullptr;                     // the second input (rtpe_hrnet_forward_aux)
  uint32_t flags = 0;                            // RTPE_FWD_*
  const int32_t* ext = nullptr;                  // a mixed-size batch: the extent table on the device
  float* op_ms = nullptr;                        // a timed forward (host-returning): the per-op times, room for n_ms of them
  int n_ms = 0;
  rtpe_record* rec = nullptr;                    // a recorded forward: the events stay with the handle
};

static FwdCall fwd_call(const void* x, int x_dtype, int N, int H, int W, void* preds, void* refined, int out_dtype, void* ws,
                        size_t ws_bytes, void* stream) {
  FwdCall c;
  c.x = x; c.x_dtype = x_dtype; c.N = N; c.H = H; c.W = W;
  c.preds = preds; c.refined = refined; c.out_dtype = out_dtype;
  c.ws = ws; c.ws_bytes = ws_bytes; c.stream = reinterpret_cast<hipStream_t>(stream);
  return c;
}

// What the ops cannot take is refused here, before the first launch, so that no half-run forward is left behind
static int check_ops(const Fwd& f, const FwdCall& c) {
  const rtpe_hrnet* h = f.h;
  RTPE_REQUIRE(c.op_ms == nullptr || c.n_ms >= (int)h->ops.size(), "forward_timed: op_ms too small");
  // avgpool: the kernel writes ceil(Hi / 2) x ceil(Wi / 2) pixels, the output tensor holds extent(H, ds) x extent(W, ds): a
  // map with an odd side (1 x 1, 2 x 1) of an input that is a multiple of 32 would be written beyond its tensor (a ragged
  // input's tensors hold the ceil)
  for (size_t i = 0; i < h->ops.size(); ++i) {
    const rtpe_op_desc& d = h->ops[i].d;
    if (d.kind != RTPE_OP_AVGPOOL) continue;
    const int Hi = extent(f.H, h->tensors[d.in_t].ds_log2), Wi = extent(f.W, h->tensors[d.in_t].ds_log2);
    const int Ho = extent(f.H, h->tensors[d.out_t].ds_log2), Wo = extent(f.W, h->tensors[d.out_t].ds_log2);
    RTPE_REQUIRE((Hi + 1) / 2 == Ho && (Wi + 1) / 2 == Wo,
                 "avgpool: a %d x %d map does not pool into the %d x %d output tensor", Hi, Wi, Ho, Wo);
  }
  // the fp16 forms of avgpool, se, cam_combine and sigmoid_add (an op of these kinds without RTPE_F_F32: the half body of
  // AttentionStudent) move rows in 16-byte pieces of 8 halves: every tensor they touch is an fp16 tensor whose row, channel
  // offset and channel count are multiples of 8; the SE limits are those of the fp32 form
  for (size_t i = 0; i < h->ops.size(); ++i) {
    const rtpe_op_desc& d = h->ops[i].d;
    if ((d.flags & RTPE_F_F32) || (d.kind != RTPE_OP_AVGPOOL && d.kind != RTPE_OP_SE && d.kind != RTPE_OP_CAM_COMBINE &&
                                   d.kind != RTPE_OP_SIGMOID_ADD)) continue;
    const int ts[4] = {d.in_t, d.out_t, d.kind == RTPE_OP_SE || d.kind == RTPE_OP_AVGPOOL ? -1 : d.res_t,
                       d.kind == RTPE_OP_CAM_COMBINE ? d.term_t[0] : -1};
    for (int k = 0; k < 4; ++k) {
      if (ts[k] < 0) continue;
      const rtpe_tensor_desc& t = h->tensors[ts[k]];
      const bool row = k == 0 && d.kind == RTPE_OP_SIGMOID_ADD;     // (the logits: one half per pixel is read, any row will do)
      RTPE_REQUIRE(t.reserved != 4 && (row || t.channels % 8 == 0), "op %zu: the fp16 form of this op needs fp16 tensors with rows of a "
                   "multiple of 8 channels (tensor %d: %d channels of %d bytes)", i, ts[k], t.channels, t.reserved == 4 ? 4 : 2);
      const int coff = k == 0 ? d.in_coff : k == 1 ? d.out_coff : k == 2 ? d.res_coff : 0;
      RTPE_REQUIRE(row || d.kind == RTPE_OP_SE || (coff >= 0 && coff + d.cout <= t.channels),
                   "op %zu: channels [%d, %d) do not fit tensor %d of %d channels", i, coff, coff + d.cout, ts[k], t.channels);
    }
    RTPE_REQUIRE(d.in_coff % 8 == 0 && d.out_coff % 8 == 0 && d.res_coff % 8 == 0, "op %zu: channel offsets must be multiples of 8", i);
    if (d.kind == RTPE_OP_SE) {
      RTPE_REQUIRE(d.cin > 0 && d.cout > 0 && d.cin <= 512 && d.cout <= 128, "se: C=%d hidden=%d unsupported", d.cin, d.cout);
      RTPE_REQUIRE(h->tensors[d.in_t].channels >= (d.cin + 7) / 8 * 8 && h->tensors[d.out_t].channels >= d.cin,
                   "se: rows of %d and %d halves for C=%d", h->tensors[d.in_t].channels, h->tensors[d.out_t].channels, d.cin);
    } else {
      RTPE_REQUIRE(d.cout > 0 && d.cout % 8 == 0, "op %zu: the fp16 form of this op needs a channel count that is a multiple of 8 (%d)", i, d.cout);
    }
  }
  // the fp16 forms of aux_pack, resize and gate_mul (the half body of AttentionStudentStepsHalf): the same rule - fp16 tensors,
  // rows, offsets and channel counts in multiples of 8; gate_mul's logits (in_t) are read one half per pixel
  for (size_t i = 0; i < h->ops.size(); ++i) {
    const rtpe_op_desc& d = h->ops[i].d;
    if ((d.flags & RTPE_F_F32) || (d.kind != RTPE_OP_AUX_PACK && d.kind != RTPE_OP_RESIZE && d.kind != RTPE_OP_GATE_MUL)) continue;
    const int ts[3] = {d.kind == RTPE_OP_AUX_PACK ? -1 : d.in_t, d.out_t, d.kind == RTPE_OP_GATE_MUL ? d.res_t : -1};
    for (int k = 0; k < 3; ++k) {
      if (ts[k] < 0) continue;
      const rtpe_tensor_desc& t = h->tensors[ts[k]];
      const bool row = k == 0 && d.kind == RTPE_OP_GATE_MUL;
      RTPE_REQUIRE(t.reserved != 4 && (row || t.channels % 8 == 0), "op %zu: the fp16 form of this op needs fp16 tensors with rows of a "
                   "multiple of 8 channels (tensor %d: %d channels of %d bytes)", i, ts[k], t.channels, t.reserved == 4 ? 4 : 2);
      const int coff = k == 0 ? d.in_coff : k == 1 ? d.out_coff : d.res_coff;
      RTPE_REQUIRE(row || (coff >= 0 && coff + d.cout <= t.channels),
                   "op %zu: channels [%d, %d) do not fit tensor %d of %d channels", i, coff, coff + d.cout, ts[k], t.channels);
    }
    RTPE_REQUIRE(d.in_coff % 8 == 0 && d.out_coff % 8 == 0 && d.res_coff % 8 == 0, "op %zu: channel offsets must be multiples of 8", i);
    RTPE_REQUIRE(d.cout > 0 && d.cout % 8 == 0, "op %zu: the fp16 form of this op needs a channel count that is a multiple of 8 (%d)", i, d.cout);
  }
  // what the call must bring for an op: the second input, and an fp32 `preds` for the sigmoid map that sigmoid_add and
  // gate_mul emit
  for (const OpState& o : h->ops) {
    const rtpe_op_desc& d = o.d;
    RTPE_REQUIRE(d.kind != RTPE_OP_AUX_PACK || c.aux != nullptr, "forward: this program has a second input (use rtpe_hrnet_forward_aux)");
    const bool emits = (d.kind == RTPE_OP_SIGMOID_ADD || d.kind == RTPE_OP_GATE_MUL) && (d.flags & RTPE_F_OUT_PREDS);
    RTPE_REQUIRE(!emits || (c.preds != nullptr && c.out_dtype == RTPE_DTYPE_F32), "forward: the sigmoid map output must be a float32 buffer");
  }
  return RTPE_OK;
}

// ---- the launch of one op: launch_op()'s switch and the helpers that build its argument blocks -----------------------------
static const _Float16* op_weights(const rtpe_hrnet* h, const OpState& o) { return reinterpret_cast<const _Float16*>(h->arena + o.w_dev_off[0]); }
static const float* op_affine(const rtpe_hrnet* h, const OpState& o) { return reinterpret_cast<const float*>(h->arena + o.ab_dev_off); }

static StemArgs stem_args(const Fwd& f, const FwdCall& c, size_t i) {
  const OpState& o = f.h->ops[i];
  const rtpe_op_desc& d = o.d;
  StemArgs a;
  a.x = c.x; a.x_f32 = c.x_dtype == RTPE_DTYPE_F32;
  a.w = op_weights(f.h, o);
  a.alpha = op_affine(f.h, o);
  a.beta = a.alpha + 64;
  a.y = f.tptr(d.out_t, d.out_coff);
  a.N = f.N; a.H = f.H; a.W = f.W; a.out_ld = f.h->tensors[d.out_t].channels;
  a.f32 = (d.flags & RTPE_F_F32) ? 1 : 0;
  a.ext = f.ext ? f.level(0) : nullptr;
  return a;
}

// conv1 + bn1 + relu + conv2 + bn2 + relu in one kernel: the half-resolution map stays in LDS (stem_fused.hip); or,
// option "fused_stem" = 2 (`with_conv2` false), the stem op alone on that kernel's conv1 code (the chain on the matrix pipe),
// output to memory - the bit-identity test of that chain against the VALU kernel
static StemFusedArgs stem_fused_args(const Fwd& f, const FwdCall& c, size_t i, bool with_conv2) {
  const rtpe_hrnet* h = f.h;
  const OpState& o = h->ops[i];
  const rtpe_op_desc& d = o.d;
  StemFusedArgs a;
  memset(&a, 0, sizeof(a));
  a.x = c.x; a.x_f32 = c.x_dtype == RTPE_DTYPE_F32;
  a.w1 = op_weights(h, o);
  a.alpha1 = op_affine(h, o);
  a.beta1 = a.alpha1 + 64;
  a.N = f.N; a.H = f.H; a.W = f.W;
  if (with_conv2) {
    const OpState& o2 = h->ops[i + 1];
    const rtpe_op_desc& d2 = o2.d;
    a.w2 = op_weights(h, o2);
    a.alpha2 = op_affine(h, o2);
    a.beta2 = a.alpha2 + o2.plan[0].cout_pad;
    a.y = f.tptr(d2.out_t, d2.out_coff);
    a.out_ld = h->tensors[d2.out_t].channels;
    a.relu = (d2.flags & RTPE_F_RELU) ? 1 : 0;
    a.round_conv = (d2.flags & RTPE_F_ROUND_CONV) ? 1 : 0;
  } else {
    a.y1 = f.tptr(d.out_t, d.out_coff);
    a.out_ld = h->tensors[d.out_t].channels;
  }
  return a;
}

// a fused BasicBlock (conv_block.hip): this conv and the next one
static int launch_block(const Fwd& f, size_t i, hipStream_t s) {
  const rtpe_hrnet* h = f.h;
  const OpState &o = h->ops[i], &o2 = h->ops[i + 1];
  const rtpe_op_desc& d = o.d;
  const rtpe_tensor_desc& ti = h->tensors[d.in_t];
  const int Hi = extent(f.H, ti.ds_log2), Wi = extent(f.W, ti.ds_log2);
  return conv_block_launch(f.tptr(d.in_t, d.in_coff), ti.channels, ((size_t)f.N * Hi * Wi * ti.channels - (size_t)d.in_coff) * 2,
                           f.tptr(o2.d.out_t, o2.d.out_coff), h->tensors[o2.d.out_t].channels, op_weights(h, o), op_affine(h, o),
                           op_weights(h, o2), op_affine(h, o2), f.N, Hi, Wi, s);
}

static int launch_fuse(const Fwd& f, size_t i, hipStream_t s) {
  const rtpe_hrnet* h = f.h;
  const rtpe_op_desc& d = h->ops[i].d;
  const rtpe_tensor_desc& to = h->tensors[d.out_t];
  FuseArgs a;
  memset(&a, 0, sizeof(a));
  a.n_terms = d.n_terms;
  for (int t = 0; t < d.n_terms; ++t) {
    const rtpe_tensor_desc& tt = h->tensors[d.term_t[t]];
    a.term[t] = f.tptr(d.term_t[t], 0);
    a.term_ld[t] = tt.channels;
    a.term_up[t] = d.term_up[t];
    a.term_h[t] = extent(f.H, tt.ds_log2);
    a.term_w[t] = extent(f.W, tt.ds_log2);
    if (f.ext) a.ext_term[t] = f.level(tt.ds_log2);
  }
  a.y = f.tptr(d.out_t, d.out_coff);
  a.out_ld = to.channels; a.C = d.cout;
  a.N = f.N; a.H = extent(f.H, to.ds_log2); a.W = extent(f.W, to.ds_log2);
  a.nearest = f.rag ? 1 : 0;
  if (f.ext) a.ext_out = f.level(to.ds_log2);
  a.f32 = (d.flags & RTPE_F_F32) ? 1 : 0;
  a.relu = (d.flags & RTPE_F_RELU) ? 1 : 0;
  return fuse_launch(a, s);
}

// cast (fp16 -> fp32), and the ops of the second input on tensors of T - aux_pack, resize, gate_mul: float, or _Float16 for the
// half body of AttentionStudentStepsHalf (whose conditions check_ops holds); the launch functions are overloaded on the pointer type
template <typename T>
static int launch_aux_op(const Fwd& f, const FwdCall& c, size_t i, hipStream_t s) {
  const rtpe_hrnet* h = f.h;
  const rtpe_op_desc& d = h->ops[i].d;
  const rtpe_tensor_desc& to = h->tensors[d.out_t];
  const int N = f.N, Ho = extent(f.H, to.ds_log2), Wo = extent(f.W, to.ds_log2);
  T* y = reinterpret_cast<T*>(f.tptr(d.out_t, d.out_coff));
  if (d.kind == RTPE_OP_AUX_PACK) return aux_pack_launch(reinterpret_cast<const float*>(c.aux), y, to.channels, N, Ho, Wo, s);
  const rtpe_tensor_desc& ti = h->tensors[d.in_t];
  const int Hi = extent(f.H, ti.ds_log2), Wi = extent(f.W, ti.ds_log2);
  const size_t pixels = (size_t)N * Hi * Wi;
  if (d.kind == RTPE_OP_CAST)
    return cast_launch(f.tptr(d.in_t, d.in_coff), ti.channels, reinterpret_cast<float*>(f.tptr(d.out_t, d.out_coff)), to.channels, d.cout,
                       pixels, s);
  const T* x = reinterpret_cast<const T*>(f.tptr(d.in_t, d.in_coff));
  if (d.kind == RTPE_OP_RESIZE)       // (a mixed-size batch: image n's own scale, clamp and extent, from its rows of the table)
    return resize_nhwc_launch(x, ti.channels, Hi, Wi, y, to.channels, Ho, Wo, d.cout, N, s, f.ext ? f.level(ti.ds_log2) : nullptr,
                              f.ext ? f.level(to.ds_log2) : nullptr);
  float div;                                     // gate_mul
  memcpy(&div, &d.reserved[0], sizeof(float));
  return gate_mul_launch(x, ti.channels, reinterpret_cast<const T*>(f.tptr(d.res_t, d.res_coff)), h->tensors[d.res_t].channels, y,
                         to.channels, d.cout, pixels, div, (d.flags & RTPE_F_OUT_PREDS) ? reinterpret_cast<float*>(c.preds) : nullptr, s);
}

// avgpool, se, cam_combine and sigmoid_add on tensors of T: float, or _Float16 for the half body of AttentionStudent (whose
// conditions check_ops holds); the launch functions are overloaded on the pointer type
template <typename T>
static int launch_student_op(const Fwd& f, const FwdCall& c, size_t i, hipStream_t s) {
  const rtpe_hrnet* h = f.h;
  const OpState& o = h->ops[i];
  const rtpe_op_desc& d = o.d;
  const rtpe_tensor_desc &ti = h->tensors[d.in_t], &to = h->tensors[d.out_t];
  const int N = f.N, Hi = extent(f.H, ti.ds_log2), Wi = extent(f.W, ti.ds_log2);
  auto at = [&](int t, int coff) { return reinterpret_cast<T*>(f.tptr(t, coff)); };
  const T* x = at(d.in_t, d.in_coff);
  T* y = at(d.out_t, d.out_coff);
  const int* ext_in = f.ext ? f.level(ti.ds_log2) : nullptr;            // avgpool, se: image n's own part of the map
  switch (d.kind) {
    case RTPE_OP_AVGPOOL:
      return avgpool_launch(x, ti.channels, y, to.channels, d.cout, N, Hi, Wi, s, ext_in);
    case RTPE_OP_SE:
      return se_launch(x, ti.channels, d.cin, d.cout, N, Hi * Wi, reinterpret_cast<const float*>(h->arena + o.w_dev_off[0]), y,
                       to.channels, s, ext_in, Wi);
    case RTPE_OP_CAM_COMBINE:
      return cam_combine_launch(x, ti.channels, at(d.res_t, d.res_coff), h->tensors[d.res_t].channels, at(d.term_t[0], 0),
                                h->tensors[d.term_t[0]].channels, y, to.channels, d.cout, N, (size_t)Hi * Wi, s);
    default:   // RTPE_OP_SIGMOID_ADD
      return sigmoid_add_launch(x, ti.channels, at(d.res_t, d.res_coff), h->tensors[d.res_t].channels, y, to.channels, d.cout,
                                (size_t)N * Hi * Wi, (d.flags & RTPE_F_OUT_PREDS) ? reinterpret_cast<float*>(c.preds) : nullptr, s);
  }
}

// What the route of op i says, on stream s: one case per route kind, then the ops that have no conv by their kind
static int launch_op(const Fwd& f, const FwdCall& c, const std::vector<Route>& routes, const std::vector<ConvArgs>& args, size_t i,
                     hipStream_t s) {
  const rtpe_hrnet* h = f.h;
  const OpState& o = h->ops[i];
  const Route& r = routes[i];
  switch (r.how) {
    case kRouteDoneBy: case kRoutePairHead: case kRoutePairProj:      // computed by the launch at op r.by
      return RTPE_OK;
    case kRouteStemFused: case kRouteStemConv1:
      return stem_fused_launch(stem_fused_args(f, c, i, r.how == kRouteStemFused), s);
    case kRouteStemPlain:
      return stem_launch(stem_args(f, c, i), s);
    case kRouteBlock:
      return launch_block(f, i, s);
    case kRouteS2Group: {
      const ConvPlan* plans[3];
      for (int m = 0; m < r.by; ++m) plans[m] = &h->ops[i + m].plan[0];
      return conv48s2_launch_group(plans, &args[i], r.by, s);
    }
    case kRoutePairTail: {   // with the head and, where it is folded, the head's skip projection
      const OpState& oh = h->ops[r.by];
      const bool proj = oh.proj_op >= 0 && routes[oh.proj_op].how == kRoutePairProj;
      return conv_pair_launch(oh.plan[0], args[r.by], o.plan[0], args[i], s, proj ? &h->ops[oh.proj_op].plan[0] : nullptr,
                              proj ? &args[oh.proj_op] : nullptr);
    }
    case kRouteDeconvMerged: case kRouteDeconv48:
      return launch_conv(r.how, o.plan[0], r.tile[0], args[i], s);
    case kRouteTile: case kRouteStream: case kRouteDirect: case kRouteConv64: case kRouteHead: case kRouteS2: {
      // a conv on the kernel of its launch shape (a launch per class) or on the head / stride-2 kernel
      int rc = launch_conv(r.how, o.plan[0], r.tile[0], args[i], s);
      for (int k = 1; k < o.n_geom && rc == RTPE_OK; ++k)
        rc = launch_conv(r.how, o.plan[k], r.tile[k], conv_op_args(f, i, k, r.tile[k]), s);
      return rc;
    }
    default:                                                          // kRouteNone: the elementwise and student ops
      break;
  }
  switch (o.d.kind) {
    case RTPE_OP_CAST:
      return launch_aux_op<float>(f, c, i, s);
    case RTPE_OP_AUX_PACK: case RTPE_OP_RESIZE: case RTPE_OP_GATE_MUL:
      return (o.d.flags & RTPE_F_F32) ? launch_aux_op<float>(f, c, i, s) : launch_aux_op<_Float16>(f, c, i, s);
    case RTPE_OP_AVGPOOL: case RTPE_OP_SE: case RTPE_OP_CAM_COMBINE: case RTPE_OP_SIGMOID_ADD:
      return (o.d.flags & RTPE_F_F32) ? launch_student_op<float>(f, c, i, s) : launch_student_op<_Float16>(f, c, i, s);
    default:
      return launch_fuse(f, i, s);
  }
}

// ---- parallel regions ---------------------------------------------------------------------------------------------------
// The branches of a HighResolutionModule (pose_higher_hrnet.py:242-243) and the conversion convs of its fuse layers are
// independent: with lanes on, the ops of lane k > 0 go to an internal stream that forks from the caller's stream at the
// region's first op and joins it behind its last; an op waits for the events of the ops of other lanes whose output it reads.
// Timed / recorded runs stay on one stream (one op after another).  The lock is rtpe_hrnet::lane_mu's: taken here, given back
// when the forward returns, behind the join of its last region.
class Lanes {
 public:
  Lanes(rtpe_hrnet* h, const FwdCall& c, const std::vector<Route>& routes, std::vector<int32_t>* trace)
      : h_(h), routes_(routes), main_(c.stream), tr_(trace) {
    if (h->has_regions && c.op_ms == nullptr && c.rec == nullptr && !(c.flags & RTPE_FWD_NO_LANES)) {
      const int opt = get_option(kOptLanes);
      on_ = opt == 1 || (opt == 2 && (long long)c.N * c.H * c.W <= 4ll * 640 * 640);
    }
    if (on_) lock_ = std::unique_lock<std::mutex>(h->lane_mu);
  }
  bool on() const { return on_; }
  // the number a trace gives stream s: 0 the caller's, 1..3 the lanes'
  int stream_id(hipStream_t s) const {
    for (int l = 1; l < 4; ++l) if (on_ && s == h_->lane_stream[l] && s != main_) return l;
    return 0;
  }

  // the stream of op i, behind everything the op reads: the join of the region before it, the fork of its own, the events of
  // the other lanes' ops that it waits for
  int stream_for(size_t i, hipStream_t* s) {
    *s = main_;
    if (!on_) return RTPE_OK;
    if (h_->fork_event == nullptr) {               // the first forward with lanes on makes the handle's streams and events
      const int rc = create();
      if (rc != RTPE_OK) return rc;
    }
    const rtpe_op_desc& d = h_->ops[i].d;
    if (d.region != region_) {
      const int rc = join();
      if (rc != RTPE_OK) return rc;
      region_ = d.region;
      if (region_ > 0) {                           // fork: every lane starts behind what the caller's stream holds
        const int fork = (int)h_->ops.size() + RTPE_TRACE_FORK_EVENT;
        int rc2 = record(fork, main_);
        for (int l = 1; l < 4 && rc2 == RTPE_OK; ++l) rc2 = wait(h_->lane_stream[l], fork);
        if (rc2 != RTPE_OK) return rc2;
      }
    }
    if (region_ == 0) return RTPE_OK;
    if (d.lane > 0) { *s = h_->lane_stream[d.lane]; used_[d.lane] = true; }
    // the op's own waits and those of the ops behind it that this launch computes (a block's second conv, the stem's
    // conv2, the other convs of a stride-2 group)
    for (size_t j = i; j == i || (j < routes_.size() && routes_[j].how == kRouteDoneBy && routes_[j].by == (int)i); ++j)
      for (int w : h_->wait_ops[j]) {
        const int rc = wait(*s, w);
        if (rc != RTPE_OK) return rc;
      }
    return RTPE_OK;
  }

  // behind the launch of op i on s: the events that other lanes wait for
  int after(size_t i, hipStream_t s) {
    if (!on_ || region_ == 0) return RTPE_OK;
    const Route& r = routes_[i];
    // (a 1x1 pair is ONE kernel, launched at the tail's place: the head's output exists behind that launch)
    int rc = RTPE_OK;
    if (h_->needs_event[i] && r.how != kRoutePairHead) rc = record((int)i, s);
    if (rc == RTPE_OK && r.how == kRoutePairTail && h_->needs_event[r.by]) rc = record(r.by, s);
    return rc;
  }

  // the caller's stream waits for every lane the open region used
  int join() {
    if (!on_ || region_ == 0) return RTPE_OK;
    for (int l = 1; l < 4; ++l) {
      if (!used_[l]) continue;
      const int e = (int)h_->ops.size() + l;
      int rc = record(e, h_->lane_stream[l]);
      if (rc == RTPE_OK) rc = wait(main_, e);
      if (rc != RTPE_OK) return rc;
      used_[l] = false;
    }
    return RTPE_OK;
  }

 private:
  // Every event call of a forward goes through these two: the HIP call and, in a traced forward, its record.  Event ids
  // (rtpe_hip_trace.h): op i's event, n_ops + l for lane l's join, n_ops + RTPE_TRACE_FORK_EVENT for the fork
  hipEvent_t event(int id) const { return id == (int)h_->ops.size() + RTPE_TRACE_FORK_EVENT ? h_->fork_event : h_->op_event[id]; }
  int record(int id, hipStream_t s) {
    RTPE_HIP_CHECK(hipEventRecord(event(id), s));
    if (tr_) trace_put(tr_, RTPE_TRACE_RECORD, stream_id(s), id);
    return RTPE_OK;
  }
  int wait(hipStream_t s, int id) {
    RTPE_HIP_CHECK(hipStreamWaitEvent(s, event(id), 0));
    if (tr_) trace_put(tr_, RTPE_TRACE_WAIT, stream_id(s), id);
    return RTPE_OK;
  }

  int create() {
    const size_t n = h_->ops.size();
    for (int l = 1; l < 4; ++l) RTPE_HIP_CHECK(hipStreamCreateWithFlags(&h_->lane_stream[l], hipStreamNonBlocking));
    h_->op_event.assign(n + 4, nullptr);
    for (size_t i = 0; i < n; ++i)
      if (h_->needs_event[i]) RTPE_HIP_CHECK(hipEventCreateWithFlags(&h_->op_event[i], hipEventDisableTiming));
    for (size_t l = 0; l < 4; ++l) RTPE_HIP_CHECK(hipEventCreateWithFlags(&h_->op_event[n + l], hipEventDisableTiming));
    RTPE_HIP_CHECK(hipEventCreateWithFlags(&h_->fork_event, hipEventDisableTiming));
    return RTPE_OK;
  }

  rtpe_hrnet* h_;
  const std::vector<Route>& routes_;
  hipStream_t main_;
  std::vector<int32_t>* tr_;
  bool on_ = false;
  std::unique_lock<std::mutex> lock_;
  int region_ = 0;
  bool used_[4] = {false, false, false, false};
};

// The per-op events of a timed forward (its own: destroyed when the forward returns, however it returns) and of a recorded one
// (the handle's: rtpe_hrnet_read_record reads them later)
class OpEvents {
 public:
  explicit OpEvents(const std::vector<Route>& routes) : routes_(routes) {}
  ~OpEvents() { for (hipEvent_t e : own_) if (e) hipEventDestroy(e); }

  int begin(const FwdCall& c) {
    const size_t n = routes_.size() + 1;
    if (c.op_ms != nullptr) {
      own_.assign(n, nullptr);
      for (auto& e : own_) RTPE_HIP_CHECK(hipEventCreate(&e));
      sets_[n_sets_++] = &own_;
      RTPE_HIP_CHECK(hipEventRecord(own_[0], c.stream));
    }
    if (c.rec != nullptr) {                      // non-blocking recording into caller-kept events
      if (c.rec->ev.size() != n) {
        for (auto& e : c.rec->ev) hipEventDestroy(e);
        c.rec->ev.resize(n);
        for (auto& e : c.rec->ev) RTPE_HIP_CHECK(hipEventCreate(&e));
      }
      c.rec->routes = routes_;
      sets_[n_sets_++] = &c.rec->ev;
      RTPE_HIP_CHECK(hipEventRecord(c.rec->ev[0], c.stream));
    }
    return RTPE_OK;
  }

  // the event behind op i, where the op has one (op_has_event)
  int record(size_t i, hipStream_t s) {
    if (n_sets_ == 0 || !op_has_event(routes_, i)) return RTPE_OK;
    for (int k = 0; k < n_sets_; ++k) RTPE_HIP_CHECK(hipEventRecord((*sets_[k])[i + 1], s));
    return RTPE_OK;
  }

  // a timed forward: wait for the last event and read the times
  int read(float* op_ms) {
    if (own_.empty()) return RTPE_OK;
    RTPE_HIP_CHECK(hipEventSynchronize(own_.back()));
    return read_op_times(routes_, own_, op_ms);
  }

 private:
  const std::vector<Route>& routes_;
  std::vector<hipEvent_t> own_;
  std::vector<hipEvent_t>* sets_[2] = {nullptr, nullptr};
  int n_sets_ = 0;
};

// a mixed-size batch: whatever the forward left outside an image's own region of the two outputs becomes 0.0
static int mask_mixed_outputs(const Fwd& f, const FwdCall& c) {
  const rtpe_hrnet* h = f.h;
  float* y[2] = {nullptr, nullptr};
  int C[2] = {0, 0}, lv[2] = {0, 0};
  for (const OpState& o : h->ops) {
    const rtpe_op_desc& d = o.d;
    if (!(d.flags & (RTPE_F_OUT_PREDS | RTPE_F_OUT_REFINED))) continue;
    const int k = (d.flags & RTPE_F_OUT_REFINED) ? 1 : 0;
    y[k] = reinterpret_cast<float*>(k ? c.refined : c.preds);
    C[k] = d.kind == RTPE_OP_SIGMOID_ADD || d.kind == RTPE_OP_GATE_MUL ? 1 : d.cout;
    lv[k] = h->tensors[d.in_t].ds_log2 + (d.kind == RTPE_OP_CONV && d.stride == 2 ? 1 : 0);
  }
  for (int k = 0; k < 2; ++k) if (y[k] == nullptr) C[k] = 0;
  return mask_outputs_launch(y[0], C[0], extent(f.H, lv[0]), extent(f.W, lv[0]), f.level(lv[0]), y[1], C[1], extent(f.H, lv[1]),
                             extent(f.W, lv[1]), f.level(lv[1]), f.N, c.stream);
}

// RTPE_HOST_PROF=n: the host time of a forward and where it goes, to stderr every n forwards.  The second number is the time
// inside launch_op() and mask_mixed_outputs(): every launch helper with the building of its arguments, for every kind of op
struct HostProf {
  typedef std::chrono::steady_clock clock;
  static int every() { static const int n = env_int("RTPE_HOST_PROF", 0); return n; }
  const int on = every();
  const clock::time_point t0 = clock::now();
  double launch_us = 0.0;

  template <typename F>
  int launch(F&& fn) {
    if (!on) return fn();
    const clock::time_point t = clock::now();
    const int rc = fn();
    launch_us += std::chrono::duration<double, std::micro>(clock::now() - t).count();
    return rc;
  }

  void report(int N, size_t n_ops, bool lanes) const {
    if (!on) return;
    static double sum_total = 0.0, sum_launch = 0.0;
    static int n_calls = 0;
    sum_total += std::chrono::duration<double, std::micro>(clock::now() - t0).count();
    sum_launch += launch_us;
    if (++n_calls % on == 0) {
      fprintf(stderr, "rtpe host profile (N=%d, %zu ops, lanes %d): %.0f us per forward on the host, %.0f us of it inside the kernel "
              "launch helpers (mean of %d calls)\n", N, n_ops, (int)lanes, sum_total / n_calls, sum_launch / n_calls, n_calls);
    }
  }
};

}  // namespace

static int run(rtpe_hrnet* h, const FwdCall& c) {
  RTPE_REQUIRE(h && c.x && c.ws, "forward: null argument");
  HostProf prof;
  // kernels, events and function attributes act on HIP's CURRENT device: make the handle's device current for
  // the call (the stream and every buffer must belong to it) and give the caller's device back afterwards
  DeviceGuard guard(h->device);
  RTPE_HIP_CHECK(guard.err);
  int rc = check_shape(h, c.N, c.H, c.W, "forward", c.ext != nullptr, c.aux != nullptr);
  if (rc != RTPE_OK) return rc;
  RTPE_REQUIRE(c.x_dtype == RTPE_DTYPE_F16 || c.x_dtype == RTPE_DTYPE_F32, "forward: x dtype");
  RTPE_REQUIRE(c.out_dtype == RTPE_DTYPE_F16 || c.out_dtype == RTPE_DTYPE_F32, "forward: out dtype");
  const Fwd f(h, c.N, c.H, c.W, c.ws, c.preds, c.refined, c.out_dtype, c.ext);
  if (f.ws_need > c.ws_bytes) { set_error("forward: workspace %zu < %zu", c.ws_bytes, f.ws_need); return RTPE_E_NOMEM; }
  RTPE_REQUIRE(((uintptr_t)c.ws & 255) == 0, "forward: workspace must be 256-byte aligned");
  if ((rc = check_ops(f, c)) != RTPE_OK) return rc;
  std::vector<Route> routes;
  std::vector<ConvArgs> args;
  if ((rc = route_ops(f, &routes, &args)) != RTPE_OK) return rc;
  OpEvents events(routes);                       // nothing is enqueued above this line
  if ((rc = events.begin(c)) != RTPE_OK) return rc;
  std::vector<int32_t>* const tr = (c.flags & RTPE_FWD_TRACE) ? &h->trace : nullptr;     // (an untraced forward tests this pointer, no more)
  if (tr) tr->clear();
  Lanes lanes(h, c, routes, tr);
  for (size_t i = 0; i < h->ops.size(); ++i) {
    hipStream_t s;
    if ((rc = lanes.stream_for(i, &s)) != RTPE_OK) return rc;
    if (tr) trace_put(tr, RTPE_TRACE_LAUNCH, (int)i, lanes.stream_id(s), routes[i].how, routes[i].by);
    if ((rc = prof.launch([&] { return launch_op(f, c, routes, args, i, s); })) != RTPE_OK) return rc;
    if ((rc = lanes.after(i, s)) != RTPE_OK) return rc;
    if ((rc = events.record(i, s)) != RTPE_OK) return rc;
  }
  if ((rc = lanes.join()) != RTPE_OK) return rc;
  if (c.ext != nullptr && tr) trace_put(tr, RTPE_TRACE_MASK, 0, 0);
  if (c.ext != nullptr && (rc = prof.launch([&] { return mask_mixed_outputs(f, c); })) != RTPE_OK) return rc;
  prof.report(c.N, h->ops.size(), lanes.on());
  return events.read(c.op_ms);
}

extern "C" int rtpe_hrnet_forward(rtpe_hrnet* h, const void* x, int32_t x_dtype, int32_t N, int32_t H,
                                  int32_t W, void* preds, void* refined, int32_t out_dtype, void* workspace,
                                  size_t workspace_bytes, void* stream) {
  return run(h, fwd_call(x, x_dtype, N, H, W, preds, refined, out_dtype, workspace, workspace_bytes, stream));
}

extern "C" int rtpe_hrnet_forward_flags(rtpe_hrnet* h, const void* x, int32_t x_dtype, int32_t N, int32_t H,
                                        int32_t W, void* preds, void* refined, int32_t out_dtype, void* workspace,
                                        size_t workspace_bytes, void* stream, uint32_t flags) {
  RTPE_REQUIRE((flags & ~(uint32_t)(RTPE_FWD_NO_LANES | RTPE_FWD_TRACE)) == 0, "forward_flags: unknown flag bits 0x%x", flags);
  FwdCall c = fwd_call(x, x_dtype, N, H, W, preds, refined, out_dtype, workspace, workspace_bytes, stream);
  c.flags = flags;
  return run(h, c);
}

extern "C" int rtpe_hrnet_forward_aux(rtpe_hrnet* h, const void* x, int32_t x_dtype, const void* aux_nchw_f32, int32_t N,
                                      int32_t H, int32_t W, void* preds, void* refined, int32_t out_dtype,
                                      void* workspace, size_t workspace_bytes, void* stream) {
  RTPE_REQUIRE(aux_nchw_f32 != nullptr, "forward_aux: the second input is null");
  FwdCall c = fwd_call(x, x_dtype, N, H, W, preds, refined, out_dtype, workspace, workspace_bytes, stream);
  c.aux = aux_nchw_f32;
  return run(h, c);
}

// ---- the trace of a forward (include/rtpe_hip_trace.h) ---------------------
extern "C" int rtpe_hrnet_forward_aux_flags(rtpe_hrnet* h, const void* x, int32_t x_dtype, const void* aux_nchw_f32, int32_t N,
                                            int32_t H, int32_t W, void* preds, void* refined, int32_t out_dtype,
                                            void* workspace, size_t workspace_bytes, void* stream, uint32_t flags) {
  RTPE_REQUIRE(aux_nchw_f32 != nullptr, "forward_aux_flags: the second input is null");
  RTPE_REQUIRE((flags & ~(uint32_t)(RTPE_FWD_NO_LANES | RTPE_FWD_TRACE)) == 0, "forward_aux_flags: unknown flag bits 0x%x", flags);
  FwdCall c = fwd_call(x, x_dtype, N, H, W, preds, refined, out_dtype, workspace, workspace_bytes, stream);
  c.aux = aux_nchw_f32;
  c.flags = flags;
  return run(h, c);
}

extern "C" int rtpe_hrnet_read_trace(const rtpe_hrnet* h, int32_t* out, int32_t n_ints, int32_t* count) {
  RTPE_REQUIRE(h != nullptr && count != nullptr, "read_trace: null argument");
  *count = (int32_t)h->trace.size();
  if (out == nullptr) return RTPE_OK;
  RTPE_REQUIRE(n_ints >= *count, "read_trace: room for %d integers, the trace has %d", n_ints, *count);
  if (*count) memcpy(out, h->trace.data(), h->trace.size() * sizeof(int32_t));
  return RTPE_OK;
}

extern "C" int rtpe_hrnet_forward_timed(rtpe_hrnet* h, const void* x, int32_t x_dtype, int32_t N, int32_t H,
                                        int32_t W, void* preds, void* refined, int32_t out_dtype,
                                        void* workspace, size_t workspace_bytes, void* stream, float* op_ms,
                                        int32_t n_ops) {
  RTPE_REQUIRE(op_ms != nullptr, "forward_timed: op_ms is null");
  FwdCall c = fwd_call(x, x_dtype, N, H, W, preds, refined, out_dtype, workspace, workspace_bytes, stream);
  c.op_ms = op_ms;
  c.n_ms = n_ops;
  return run(h, c);
}

extern "C" int rtpe_hrnet_op_cost(const rtpe_hrnet* h, int32_t op, int32_t N, int32_t H, int32_t W,
                                  double* flops, double* bytes) {
  RTPE_REQUIRE(h && op >= 0 && op < (int)h->ops.size() && flops && bytes, "op_cost: bad argument");
  const rtpe_op_desc& d = h->ops[op].d;
  *flops = 0; *bytes = 0;
  if (d.kind == RTPE_OP_FUSE) {
    const rtpe_tensor_desc& to = h->tensors[d.out_t];
    const double px = (double)N * extent(H, to.ds_log2) * extent(W, to.ds_log2);
    *bytes = px * d.cout * 2;
    for (int t = 0; t < d.n_terms; ++t) *bytes += px / (double)(1 << (2 * d.term_up[t])) * d.cout * 2;
    return RTPE_OK;
  }
  const int cin_logical = d.reserved[0] > 0 ? d.reserved[0] : d.cin;
  if (d.kind >= RTPE_OP_CAST) {                      // small student ops: bytes only
    const rtpe_tensor_desc& ti = h->tensors[d.kind == RTPE_OP_AUX_PACK ? d.out_t : d.in_t];
    const double px = (double)N * extent(H, ti.ds_log2) * extent(W, ti.ds_log2);
    *bytes = px * ti.channels * ((d.flags & RTPE_F_F32) ? 4 : 2) * 2;
    return RTPE_OK;
  }
  if (d.kind == RTPE_OP_STEM) {
    const double po = (double)N * extent(H, 1) * extent(W, 1);
    *flops = 2.0 * po * 64 * 27;
    *bytes = (double)N * 3 * H * W * 4 + po * 64 * 2;
    return RTPE_OK;
  }
  const rtpe_tensor_desc& ti = h->tensors[d.in_t];
  const double pi = (double)N * extent(H, ti.ds_log2) * extent(W, ti.ds_log2);
  const bool dc = d.kind == RTPE_OP_DECONV;
  const double po = dc ? pi * 4 : (double)N * conv_pos(h, d, H) * conv_pos(h, d, W);
  const double taps = dc ? 4 : d.ksize * d.ksize;
  const double es = (d.flags & RTPE_F_F32) ? 4.0 : 2.0;       // bytes per element of this op's tensors
  *flops = 2.0 * po * d.cout * cin_logical * taps;
  *bytes = pi * cin_logical * es + po * d.cout * es + (d.res_t >= 0 ? po * d.cout * es : 0) +
           (double)cin_logical * d.cout * d.ksize * d.ksize * es;
  return RTPE_OK;
}

// ---- ragged shapes (include/rtpe_hip_anysize.h) ----------------------------
extern "C" int32_t rtpe_extent(int32_t n, int32_t ds_log2) { return n > 0 && ds_log2 >= 0 && ds_log2 < 31 ? extent(n, ds_log2) : 0; }

extern "C" int32_t rtpe_nearest_src(int32_t dst, int32_t n_in, int32_t n_out) {
  return dst >= 0 && n_in > 0 && dst < n_out ? nearest_src(dst, n_in, (float)n_in / (float)n_out) : -1;
}

extern "C" int rtpe_hrnet_set_any_size(rtpe_hrnet* h, int32_t on) {
  RTPE_REQUIRE(h != nullptr && (on == 0 || on == 1), "set_any_size: bad argument");
  h->any_size = on != 0;
  return RTPE_OK;
}

extern "C" int rtpe_hrnet_get_any_size(const rtpe_hrnet* h, int32_t* on) {
  RTPE_REQUIRE(h != nullptr && on != nullptr, "get_any_size: null argument");
  *on = h->any_size ? 1 : 0;
  return RTPE_OK;
}

// ---- mixed-size batches (include/rtpe_hip_mixed.h) -------------------------
static size_t mixed_table_bytes(int N) { return align_up((size_t)RTPE_MIXED_LEVELS * 2 * N * sizeof(int32_t), 256); }

extern "C" int rtpe_mixed_table_ints(int32_t N, int32_t* count) {
  RTPE_REQUIRE(N > 0 && N <= (1 << 20) && count != nullptr, "mixed_table_ints: N=%d", N);
  *count = RTPE_MIXED_LEVELS * 2 * N;
  return RTPE_OK;
}

extern "C" int rtpe_mixed_table_fill(const int32_t* sizes_hw, int32_t N, int32_t Hc, int32_t Wc, int32_t* table, int32_t n_ints) {
  RTPE_REQUIRE(sizes_hw != nullptr && table != nullptr && N > 0 && N <= (1 << 20), "mixed_table_fill: null argument or N=%d", N);
  RTPE_REQUIRE(n_ints >= RTPE_MIXED_LEVELS * 2 * N, "mixed_table_fill: %d integers for %d images (%d needed)", n_ints, N,
               RTPE_MIXED_LEVELS * 2 * N);
  RTPE_REQUIRE(Hc >= 32 && Wc >= 32, "mixed_table_fill: canvas %d x %d", Hc, Wc);
  for (int n = 0; n < N; ++n) {
    const int hn = sizes_hw[2 * n], wn = sizes_hw[2 * n + 1];
    RTPE_REQUIRE(hn >= 32 && wn >= 32, "mixed_table_fill: image %d is %d x %d, both sides must be at least 32", n, hn, wn);
    RTPE_REQUIRE(hn <= Hc && wn <= Wc, "mixed_table_fill: image %d is %d x %d, larger than the %d x %d canvas", n, hn, wn, Hc, Wc);
  }
  for (int d = 0; d < RTPE_MIXED_LEVELS; ++d)
    for (int n = 0; n < N; ++n) {
      table[((size_t)d * N + n) * 2] = extent(sizes_hw[2 * n], d);
      table[((size_t)d * N + n) * 2 + 1] = extent(sizes_hw[2 * n + 1], d);
    }
  return RTPE_OK;
}

extern "C" int rtpe_hrnet_mixed_workspace_bytes(const rtpe_hrnet* h, int32_t N, int32_t Hc, int32_t Wc, size_t* bytes) {
  RTPE_REQUIRE(h != nullptr && bytes != nullptr, "mixed_workspace_bytes: null argument");
  {
    const int rc = check_shape(h, N, Hc, Wc, "mixed_workspace_bytes", true, /*aux_ok=*/true);
    if (rc != RTPE_OK) return rc;
  }
  std::vector<size_t> offs;
  slot_layout(h, N, Hc, Wc, &offs, bytes);
  *bytes = align_up(*bytes, 256) + mixed_table_bytes(N);
  return RTPE_OK;
}

// both entries: `aux` is the second input's canvas, or null for a program that has none
static int forward_mixed(rtpe_hrnet* h, const void* x, int32_t x_dtype, const void* aux, int32_t N, int32_t Hc, int32_t Wc,
                         const int32_t* sizes_hw, int32_t* table_pinned, int32_t table_ints, void* preds, void* refined,
                         int32_t out_dtype, void* workspace, size_t workspace_bytes, void* stream, uint32_t flags) {
  RTPE_REQUIRE(h && x && workspace && sizes_hw && table_pinned, "forward_mixed: null argument");
  RTPE_REQUIRE((flags & ~(uint32_t)(RTPE_FWD_NO_LANES | RTPE_FWD_TRACE)) == 0, "forward_mixed: unknown flag bits 0x%x", flags);
  RTPE_REQUIRE(out_dtype == RTPE_DTYPE_F32, "forward_mixed: the outputs are float32 buffers");
  // everything that can be refused is refused here, before the table leaves the host
  int rc = check_shape(h, N, Hc, Wc, "forward_mixed", true, aux != nullptr);
  if (rc != RTPE_OK) return rc;
  if (aux != nullptr) {
    bool has_aux = false;
    for (const OpState& o : h->ops) has_aux = has_aux || o.d.kind == RTPE_OP_AUX_PACK;
    RTPE_REQUIRE(has_aux, "forward_mixed_aux: this program has no second input (use rtpe_hrnet_forward_mixed)");
  }
  rc = rtpe_mixed_table_fill(sizes_hw, N, Hc, Wc, table_pinned, table_ints);
  if (rc != RTPE_OK) return rc;
  std::vector<size_t> offs;
  size_t ws_need = 0;
  slot_layout(h, N, Hc, Wc, &offs, &ws_need);
  ws_need = align_up(ws_need, 256);
  if (ws_need + mixed_table_bytes(N) > workspace_bytes) {
    set_error("forward_mixed: workspace %zu < %zu", workspace_bytes, ws_need + mixed_table_bytes(N));
    return RTPE_E_NOMEM;
  }
  RTPE_REQUIRE(((uintptr_t)workspace & 255) == 0, "forward_mixed: workspace must be 256-byte aligned");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  int32_t* table_dev = reinterpret_cast<int32_t*>(reinterpret_cast<char*>(workspace) + ws_need);
  {
    DeviceGuard guard(h->device);
    RTPE_HIP_CHECK(guard.err);
    // in stream order, from the caller's pinned block: nothing blocks, nothing is allocated
    RTPE_HIP_CHECK(hipMemcpyAsync(table_dev, table_pinned, (size_t)RTPE_MIXED_LEVELS * 2 * N * sizeof(int32_t), hipMemcpyHostToDevice, s));
  }
  FwdCall c = fwd_call(x, x_dtype, N, Hc, Wc, preds, refined, out_dtype, workspace, ws_need, stream);
  c.flags = flags;
  c.ext = table_dev;
  c.aux = aux;
  return run(h, c);
}

extern "C" int rtpe_hrnet_forward_mixed(rtpe_hrnet* h, const void* x, int32_t x_dtype, int32_t N, int32_t Hc, int32_t Wc,
                                        const int32_t* sizes_hw, int32_t* table_pinned, int32_t table_ints, void* preds,
                                        void* refined, int32_t out_dtype, void* workspace, size_t workspace_bytes, void* stream,
                                        uint32_t flags) {
  return forward_mixed(h, x, x_dtype, nullptr, N, Hc, Wc, sizes_hw, table_pinned, table_ints, preds, refined, out_dtype, workspace,
                       workspace_bytes, stream, flags);
}

// ---- ... of a program with a second input (include/rtpe_hip_mixed_aux.h) ----
extern "C" int rtpe_hrnet_forward_mixed_aux(rtpe_hrnet* h, const void* x, int32_t x_dtype, const void* aux_nchw_f32, int32_t N,
                                            int32_t Hc, int32_t Wc, const int32_t* sizes_hw, int32_t* table_pinned,
                                            int32_t table_ints, void* preds, void* refined, int32_t out_dtype, void* workspace,
                                            size_t workspace_bytes, void* stream, uint32_t flags) {
  RTPE_REQUIRE(aux_nchw_f32 != nullptr, "forward_mixed_aux: the second input is null");
  return forward_mixed(h, x, x_dtype, aux_nchw_f32, N, Hc, Wc, sizes_hw, table_pinned, table_ints, preds, refined, out_dtype,
                       workspace, workspace_bytes, stream, flags);
}

// ---- single-layer entry (layer-level parity tests) -------------------------
extern "C" int rtpe_conv2d_nhwc_ex(const void* x, int32_t N, int32_t H, int32_t W, int32_t cin,
                                   const void* w_host, const float* alpha_host, const float* beta_host,
                                   int32_t cout, int32_t ksize, int32_t stride, int32_t dilation, int32_t flags,
                                   const void* res, void* y, void* stream) {
  RTPE_REQUIRE(x && w_host && alpha_host && beta_host && y, "conv2d_nhwc: null argument");
  const int es = (flags & RTPE_F_F32) ? 4 : 2, eps = 16 / es;
  RTPE_REQUIRE((ksize == 1 || ksize == 3 || ksize == 5) && (stride == 1 || stride == 2) && cin % eps == 0 && cout % eps == 0 &&
                   dilation >= 1 && (dilation == 1 || (ksize == 3 && stride == 1)),
               "conv2d_nhwc: k=%d s=%d d=%d cin=%d cout=%d unsupported", ksize, stride, dilation, cin, cout);
  RTPE_REQUIRE(H % stride == 0 && W % stride == 0, "conv2d_nhwc: H, W must be multiples of the stride");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  ConvGeom g{cin, cout, ksize, stride, -1, es, dilation};
  ConvPlan p = conv_make_plan(g);
  std::vector<char> packed(p.packed_bytes);
  conv_pack_weights(g, p, w_host, packed.data());
  std::vector<float> ab(2 * p.cout_pad, 0.f);
  for (int c = 0; c < cout; ++c) { ab[c] = alpha_host[c]; ab[p.cout_pad + c] = beta_host[c]; }
  char* dev = nullptr;
  const size_t wb = align_up(p.packed_bytes, 256);
  RTPE_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&dev), wb + ab.size() * 4));
  hipError_t e = hipMemcpy(dev, packed.data(), p.packed_bytes, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(dev + wb, ab.data(), ab.size() * 4, hipMemcpyHostToDevice);
  if (e != hipSuccess) { hipFree(dev); return hip_fail(e, "hipMemcpy", __FILE__, __LINE__); }
  ConvArgs a;
  memset(&a, 0, sizeof(a));
  a.x = reinterpret_cast<const _Float16*>(x); a.in_ld = cin;
  a.x_bytes = (size_t)N * H * W * cin * es;
  a.w = reinterpret_cast<const _Float16*>(dev);
  a.alpha = reinterpret_cast<const float*>(dev + wb); a.beta = a.alpha + p.cout_pad;
  a.res = reinterpret_cast<const _Float16*>(res); a.res_ld = cout;
  a.y = reinterpret_cast<_Float16*>(y); a.out_ld = cout; a.cout_store = cout;
  a.N = N; a.H_in = H; a.W_in = W;
  a.H_full = a.H_pos = H / stride; a.W_full = a.W_pos = W / stride; a.o_mul = 1;
  a.relu = (flags & RTPE_F_RELU) ? 1 : 0;
  a.round_conv = (flags & RTPE_F_ROUND_CONV) ? 1 : 0;
  const RouteOpts opt;
  ConvTile tile = conv_make_tile(p, N, a.H_pos, a.W_pos);
  conv_fix_tile(opt, p, a, /*plane_io=*/false, &tile);
  // diagnostic builds, RTPE_PROBE_PLANE=1: time a streaming launch with plane-major views ([C/48][N][H][W][48], what the
  // engine gives the inner tensors of the C >= 96 block chains) over the same bytes - the values are then meaningless
  static const int probe_plane = RTPE_DIAG_ENV_INT("RTPE_PROBE_PLANE", 0);
  if (probe_plane && tile.kind == 2 && cin % 48 == 0 && cout % 48 == 0 && stride == 1) {
    a.in_ld = 48; a.in_cs = (long long)N * H * W * 48;
    a.out_ld = 48; a.out_cs = (long long)N * H * W * 48;
    if (res != nullptr) { a.res_ld = 48; a.res_cs = (long long)N * H * W * 48; }
  }
  conv_fill_args(g, p, tile, &a);
#ifdef RTPE_CONV_STAMPS
  unsigned long long* dbg = nullptr;
  hipMalloc(reinterpret_cast<void**>(&dbg), 128);
  hipMemset(dbg, 0, 128);
  a.dbg = dbg;
#endif
  int rc = launch_conv(conv_pick(opt, p, tile, a, /*plane_io=*/false), p, tile, a, s);
  hipError_t es2 = hipStreamSynchronize(s);
#ifdef RTPE_CONV_STAMPS
  unsigned long long hd[16];
  hipMemcpy(hd, dbg, 128, hipMemcpyDeviceToHost);
  hipFree(dbg);
  if (tile.kind == 2 && hd[5] && (hd[11] = hd[11] ? hd[11] : hd[5] / tile.waves)) {
    const unsigned long long nw = (unsigned long long)tile.grid * tile.waves, units = hd[5] / p.n_cchunks;
    fprintf(stderr, "stream conv %dx%d nt%d w%d nb%d nw%d grid %d | per MFMA wave: total %llu cycles, %llu units | per stage: waitM %llu half0 %llu "
            "waitH %llu half1 %llu | per unit: E-wait %llu bn+transpose %llu res-wait %llu rows+add+store %llu load_res %llu | weight loader/stage: wait %llu issue %llu | "
            "tile loaders/stage: wait %llu issue %llu\n",
            tile.th, tile.tw, tile.nt, tile.waves, tile.n_bufs, tile.n_wslots, tile.grid, hd[15] / nw, units / nw, hd[0] / hd[5], hd[1] / hd[5],
            hd[2] / hd[5], hd[3] / hd[5], hd[12] / units, hd[13] / units, hd[4] / units, hd[14] / units, hd[10] / units, hd[6] / hd[11],
            hd[7] / hd[11], hd[8] / hd[11], hd[9] / hd[11]);
  }
  else if (hd[5])
    fprintf(stderr, "conv stamps (kind %d): n %llu | per wave(-unit) cycles: setup %llu stage/wait1 %llu kloop %llu epilogue %llu total/wait2 %llu\n",
            tile.kind, hd[5], hd[0] / hd[5], hd[1] / hd[5], hd[2] / hd[5], hd[3] / hd[5], hd[4] / hd[5]);
  if (hd[10] && tile.kind != 2)
    fprintf(stderr, "   loader per stage: vmcnt-wait %llu barrier1 %llu issue %llu barriersE+2 %llu (stages %llu)\n",
            hd[6] / hd[10], hd[7] / hd[10], hd[8] / hd[10], hd[9] / hd[10], hd[10]);
#endif
  hipFree(dev);
  if (rc != RTPE_OK) return rc;
  if (es2 != hipSuccess) return hip_fail(es2, "hipStreamSynchronize", __FILE__, __LINE__);
  return RTPE_OK;
}

extern "C" int rtpe_basicblock_nhwc(const void* x, int32_t N, int32_t H, int32_t W, const void* w1_host,
                                    const float* alpha1, const float* beta1, const void* w2_host, const float* alpha2,
                                    const float* beta2, void* y, void* stream) {
  RTPE_REQUIRE(x && w1_host && w2_host && alpha1 && beta1 && alpha2 && beta2 && y, "basicblock_nhwc: null argument");
  RTPE_REQUIRE(conv_block_supports(48, 48, H, W), "basicblock_nhwc: H=%d W=%d unsupported", H, W);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  ConvGeom g{48, 48, 3, 1, -1, 2, 1};
  ConvPlan p = conv_make_plan(g);
  const size_t wb = align_up(p.packed_bytes, 256), abb = align_up(2 * 48 * sizeof(float), 256);
  std::vector<char> host(2 * (wb + abb), 0);
  const void* ws[2] = {w1_host, w2_host};
  const float* al[2] = {alpha1, alpha2};
  const float* be[2] = {beta1, beta2};
  for (int k = 0; k < 2; ++k) {
    conv_pack_weights(g, p, ws[k], host.data() + k * (wb + abb));
    float* ab = reinterpret_cast<float*>(host.data() + k * (wb + abb) + wb);
    for (int c = 0; c < 48; ++c) { ab[c] = al[k][c]; ab[48 + c] = be[k][c]; }
  }
  char* dev = nullptr;
  RTPE_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&dev), host.size()));
  hipError_t e = hipMemcpy(dev, host.data(), host.size(), hipMemcpyHostToDevice);
  if (e != hipSuccess) { hipFree(dev); return hip_fail(e, "hipMemcpy", __FILE__, __LINE__); }
  int rc = conv_block_launch(reinterpret_cast<const _Float16*>(x), 48, (size_t)N * H * W * 48 * 2,
                             reinterpret_cast<_Float16*>(y), 48, reinterpret_cast<const _Float16*>(dev),
                             reinterpret_cast<const float*>(dev + wb), reinterpret_cast<const _Float16*>(dev + wb + abb),
                             reinterpret_cast<const float*>(dev + wb + abb + wb), N, H, W, s);
  hipError_t es = hipStreamSynchronize(s);
  hipFree(dev);
  if (rc != RTPE_OK) return rc;
  if (es != hipSuccess) return hip_fail(es, "hipStreamSynchronize", __FILE__, __LINE__);
  return RTPE_OK;
}

// conv 1x1 64 -> 256 + bn + residual + ReLU and the conv 1x1 256 -> 64 + bn + ReLU behind it as ONE launch of conv_pair.hip on
// plain NHWC tensors of any pixel count (the /4 maps of a program are multiples of 64 pixels: partial tiles are reached only here).
// The residual is `res`, or - x and the third layer given - bn(Wd . x), computed inside the kernel (`res` is then not read)
extern "C" int rtpe_conv1x1_pair_nhwc(const void* t, const void* res, const void* x, int32_t N, int32_t H, int32_t W,
                                      const void* w1_host, const float* alpha1, const float* beta1, const void* w2_host,
                                      const float* alpha2, const float* beta2, const void* wd_host, const float* alphad,
                                      const float* betad, void* y, void* u, void* stream) {
  RTPE_REQUIRE(t && w1_host && alpha1 && beta1 && w2_host && alpha2 && beta2 && y && u && N > 0 && H > 0 && W > 0,
               "conv1x1_pair_nhwc: null argument");
  RTPE_REQUIRE((x != nullptr) == (wd_host != nullptr) && (x == nullptr || (alphad && betad)) && (x != nullptr || res != nullptr),
               "conv1x1_pair_nhwc: a residual tensor, or the projection's input and layer");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const int n_layers = x ? 3 : 2;
  const int cins[3] = {64, 256, 64}, couts[3] = {256, 64, 256};
  const void* ws[3] = {w1_host, w2_host, wd_host};
  const float* al[3] = {alpha1, alpha2, alphad};
  const float* be[3] = {beta1, beta2, betad};
  ConvPlan plan[3];
  size_t off[4] = {0, 0, 0, 0};
  for (int k = 0; k < n_layers; ++k) {
    plan[k] = conv_make_plan(ConvGeom{cins[k], couts[k], 1, 1, -1, 2, 1});
    off[k + 1] = off[k] + align_up(plan[k].packed_bytes, 256) + align_up(2 * sizeof(float) * plan[k].cout_pad, 256);
  }
  std::vector<char> host(off[n_layers], 0);
  for (int k = 0; k < n_layers; ++k) {
    conv_pack_weights(ConvGeom{cins[k], couts[k], 1, 1, -1, 2, 1}, plan[k], ws[k], host.data() + off[k]);
    float* ab = reinterpret_cast<float*>(host.data() + off[k] + align_up(plan[k].packed_bytes, 256));
    for (int c = 0; c < couts[k]; ++c) { ab[c] = al[k][c]; ab[plan[k].cout_pad + c] = be[k][c]; }
  }
  char* dev = nullptr;
  RTPE_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&dev), host.size()));
  hipError_t e = hipMemcpy(dev, host.data(), host.size(), hipMemcpyHostToDevice);
  if (e != hipSuccess) { hipFree(dev); return hip_fail(e, "hipMemcpy", __FILE__, __LINE__); }
  ConvArgs a[3];
  const void* in[3] = {t, y, x};
  void* out[3] = {y, u, const_cast<void*>(x ? y : res)};     // (the folded projection's output is a name only: never written)
  for (int k = 0; k < n_layers; ++k) {
    memset(&a[k], 0, sizeof(a[k]));
    a[k].x = reinterpret_cast<const _Float16*>(in[k]); a[k].in_ld = cins[k];
    a[k].x_bytes = (size_t)N * H * W * cins[k] * 2;
    a[k].w = reinterpret_cast<const _Float16*>(dev + off[k]);
    a[k].alpha = reinterpret_cast<const float*>(dev + off[k] + align_up(plan[k].packed_bytes, 256)); a[k].beta = a[k].alpha + plan[k].cout_pad;
    a[k].y = reinterpret_cast<_Float16*>(out[k]); a[k].out_ld = couts[k]; a[k].cout_store = couts[k];
    a[k].N = N; a[k].H_in = a[k].H_full = a[k].H_pos = H; a[k].W_in = a[k].W_full = a[k].W_pos = W; a[k].o_mul = 1;
    a[k].relu = k < 2; a[k].round_conv = 1;
    a[k].cin = cins[k]; a[k].cout = couts[k];
  }
  a[0].res = reinterpret_cast<const _Float16*>(x ? y : res); a[0].res_ld = 256;
  int rc = conv_pair_launch(plan[0], a[0], plan[1], a[1], s, x ? &plan[2] : nullptr, x ? &a[2] : nullptr);
  hipError_t es = hipStreamSynchronize(s);
  hipFree(dev);
  if (rc != RTPE_OK) return rc;
  if (es != hipSuccess) return hip_fail(es, "hipStreamSynchronize", __FILE__, __LINE__);
  return RTPE_OK;
}

extern "C" int rtpe_deconv4x4s2_nhwc(const void* x, int32_t N, int32_t H, int32_t W, int32_t cin,
                                     const void* w_host, const float* alpha_host, const float* beta_host,
                                     int32_t cout, int32_t flags, void* y, void* stream) {
  RTPE_REQUIRE(x && w_host && alpha_host && beta_host && y, "deconv4x4s2_nhwc: null argument");
  RTPE_REQUIRE(cin % 8 == 0 && cout % 8 == 0 && N > 0 && H > 0 && W > 0, "deconv4x4s2_nhwc: cin=%d cout=%d", cin, cout);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  int rc = RTPE_OK;
  std::vector<char*> dev_bufs;
  ConvArgs merged;
  memset(&merged, 0, sizeof(merged));
  // as in the forward: the four classes in one launch on class 0's launch shape, or four launches
  ConvPlan plans[4];
  for (int k = 0; k < 4; ++k) plans[k] = conv_make_plan(ConvGeom{cin, cout, 4, 2, k, 2, 1});
  const ConvTile tile0 = conv_make_tile(plans[0], N, H, W);
  const bool merge = deconv_merges(plans, tile0);
  for (int k = 0; k < 4 && rc == RTPE_OK; ++k) {         // the four sub-pixel (parity) classes of the output
    ConvGeom g{cin, cout, 4, 2, k, 2, 1};
    const ConvPlan p = plans[k];
    std::vector<char> packed(p.packed_bytes);
    conv_pack_weights(g, p, w_host, packed.data());
    std::vector<float> ab(2 * p.cout_pad, 0.f);
    for (int c = 0; c < cout; ++c) { ab[c] = alpha_host[c]; ab[p.cout_pad + c] = beta_host[c]; }
    char* dev = nullptr;
    const size_t wb = align_up(p.packed_bytes, 256);
    RTPE_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&dev), wb + ab.size() * 4));
    dev_bufs.push_back(dev);
    hipError_t e = hipMemcpy(dev, packed.data(), p.packed_bytes, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(dev + wb, ab.data(), ab.size() * 4, hipMemcpyHostToDevice);
    if (e != hipSuccess) { rc = hip_fail(e, "hipMemcpy", __FILE__, __LINE__); break; }
    ConvArgs a;
    memset(&a, 0, sizeof(a));
    a.x = reinterpret_cast<const _Float16*>(x); a.in_ld = cin;
    a.x_bytes = (size_t)N * H * W * cin * 2;
    a.w = reinterpret_cast<const _Float16*>(dev);
    a.alpha = reinterpret_cast<const float*>(dev + wb); a.beta = a.alpha + p.cout_pad;
    a.y = reinterpret_cast<_Float16*>(y); a.out_ld = cout; a.cout_store = cout;
    a.N = N; a.H_in = H; a.W_in = W;
    a.H_full = 2 * H; a.W_full = 2 * W;
    a.H_pos = H; a.W_pos = W; a.o_mul = 2; a.oy_add = k >> 1; a.ox_add = k & 1;
    a.relu = (flags & RTPE_F_RELU) ? 1 : 0;
    a.round_conv = (flags & RTPE_F_ROUND_CONV) ? 1 : 0;
    const ConvTile tile = merge ? tile0 : conv_make_tile(p, N, a.H_pos, a.W_pos);
    conv_fill_args(g, p, tile, &a);
    if (merge) {
      deconv_merge_class(&merged, a, k);
      if (k == 3) rc = launch_conv(deconv_pick(RouteOpts(), plans[0], merged), plans[0], tile0, merged, s);
      continue;
    }
    rc = conv_launch(p, tile, a, s);
  }
  hipError_t es = hipStreamSynchronize(s);
  for (char* d : dev_bufs) hipFree(d);
  if (rc != RTPE_OK) return rc;
  if (es != hipSuccess) return hip_fail(es, "hipStreamSynchronize", __FILE__, __LINE__);
  return RTPE_OK;
}

extern "C" int rtpe_fuse_nhwc(const void* const* terms, const int32_t* term_up, int32_t n_terms, int32_t N, int32_t H,
                              int32_t W, int32_t C, int32_t flags, void* y, void* stream) {
  RTPE_REQUIRE(terms && term_up && y && n_terms >= 1 && n_terms <= 4, "fuse_nhwc: bad argument");
  FuseArgs a;
  memset(&a, 0, sizeof(a));
  a.n_terms = n_terms;
  for (int t = 0; t < n_terms; ++t) {
    RTPE_REQUIRE(terms[t] != nullptr && term_up[t] >= 0 && term_up[t] < 8 && H % (1 << term_up[t]) == 0 &&
                     W % (1 << term_up[t]) == 0, "fuse_nhwc: term %d", t);
    a.term[t] = reinterpret_cast<const _Float16*>(terms[t]);
    a.term_ld[t] = C;
    a.term_up[t] = term_up[t];
  }
  a.y = reinterpret_cast<_Float16*>(y);
  a.out_ld = C; a.C = C; a.N = N; a.H = H; a.W = W;
  a.f32 = (flags & RTPE_F_F32) ? 1 : 0;
  a.relu = (flags & RTPE_F_RELU) ? 1 : 0;
  return fuse_launch(a, reinterpret_cast<hipStream_t>(stream));
}

extern "C" int rtpe_conv2d_nhwc(const void* x, int32_t N, int32_t H, int32_t W, int32_t cin,
                                const void* w_host, const float* alpha_host, const float* beta_host,
                                int32_t cout, int32_t ksize, int32_t stride, int32_t flags, const void* res,
                                void* y, void* stream) {
  return rtpe_conv2d_nhwc_ex(x, N, H, W, cin, w_host, alpha_host, beta_host, cout, ksize, stride, 1,
                             flags & ~RTPE_F_F32, res, y, stream);
}

// introspection for bench / tuning: kernel variant and geometry of a conv op - the route of a forward of this shape that
// binds a workspace, fp32 `preds` and `refined` (nominal, suitably aligned addresses: nothing is dereferenced)
extern "C" int rtpe_hrnet_op_tile(const rtpe_hrnet* h, int32_t op, int32_t N, int32_t H, int32_t W, int32_t* out8) {
  RTPE_REQUIRE(h && out8 && op >= 0 && op < (int)h->ops.size(), "op_tile: bad argument");
  {
    const int rc = check_shape(h, N, H, W, "op_tile");
    if (rc != RTPE_OK) return rc;
  }
  const Fwd f(h, N, H, W, reinterpret_cast<void*>(256), reinterpret_cast<void*>(256), reinterpret_cast<void*>(256), RTPE_DTYPE_F32);
  std::vector<Route> routes;
  std::vector<ConvArgs> args;
  const int rc = route_ops(f, &routes, &args);
  if (rc != RTPE_OK) return rc;
  route_label(h, routes, op, out8);
  return RTPE_OK;
}

// Per-shape plan autotuning (the reference runs its GPU path with cudnn.benchmark = True,
// teacher_inference.py:31).  Layers that look alike form a class; in round r every class
// runs its r-th launch shape (conv_enum_tiles) inside complete, per-op-timed forward
// passes, so each shape is measured in the cache state it will really see; the shape with
// the smallest summed time wins for the class.  All shapes give bit-identical results.
// Host-returning.
static int autotune_impl(rtpe_hrnet* h, const void* x, int32_t x_dtype, const void* aux, int32_t N, int32_t H, int32_t W,
                         void* preds, void* refined, int32_t out_dtype, void* workspace, size_t workspace_bytes,
                         void* stream) {
  RTPE_REQUIRE(h != nullptr, "autotune: null handle");
  // a stream of native-size images has hundreds of shapes: ragged ones run on the default launch shapes and are never tuned
  RTPE_REQUIRE(!ragged(H, W), "autotune: N=%d H=%d W=%d: shapes with a side that is no multiple of 32 are not tuned", N, H, W);
  const auto shape = std::make_tuple(N, H, W);
  h->tuned.erase(shape);
  const size_t n_ops = h->ops.size();
  std::vector<float> ms(n_ops);
  FwdCall timed = fwd_call(x, x_dtype, N, H, W, preds, refined, out_dtype, workspace, workspace_bytes, stream);
  timed.aux = aux;
  timed.op_ms = ms.data();
  timed.n_ms = (int)n_ops;
  int rc = run(h, timed);
  if (rc != RTPE_OK) return rc;
  std::vector<Route> routes;                           // (of these forwards: no launch shape decides what is absorbed)
  std::vector<ConvArgs> args;
  rc = route_ops(Fwd(h, N, H, W, workspace, preds, refined, out_dtype), &routes, &args);
  if (rc != RTPE_OK) return rc;

  typedef std::tuple<int, int, int, int, int, int, int, int, int, int> Key;   // everything a launch shape depends on
  struct Class { std::vector<size_t> ops; std::vector<std::vector<ConvTile>> cands; std::vector<double> t; };
  std::map<Key, Class> classes;
  for (size_t i = 0; i < n_ops; ++i) {
    const OpState& o = h->ops[i];
    const rtpe_op_desc& d = o.d;
    if (o.n_geom == 0) continue;
    if (routes[i].how == kRoutePairProj) continue;      // computed inside its 1x1 pair in these forwards: nothing to time, stays untuned
    const rtpe_tensor_desc& ti = h->tensors[d.in_t];
    const Key key = std::make_tuple(d.cin, d.cout, d.ksize, d.stride, (int)d.kind, (int)ti.ds_log2, d.res_t >= 0 ? 1 : 0,
                                    (int)(d.flags & (RTPE_F_OUT_PREDS | RTPE_F_OUT_REFINED | RTPE_F_NO_NHWC | RTPE_F_F32)),
                                    (int)d.reserved[1] /* dilation: sets the halo */, (int)d.reserved[2]);
    Class& c = classes[key];
    if (c.ops.empty()) {
      const int Hp = conv_pos(h, d, H), Wp = conv_pos(h, d, W);
      c.cands.resize(o.n_geom);
      for (int k = 0; k < o.n_geom; ++k) conv_enum_tiles(o.plan[k], N, Hp, Wp, &c.cands[k]);
      size_t nc = c.cands[0].size();
      for (int k = 1; k < o.n_geom; ++k) nc = c.cands[k].size() < nc ? c.cands[k].size() : nc;
      c.t.assign(nc, 0.0);
    }
    c.ops.push_back(i);
  }
  size_t rounds = 0;
  for (auto& kv : classes) rounds = kv.second.t.size() > rounds ? kv.second.t.size() : rounds;
  std::vector<ConvTile> trial(n_ops * 4);
  for (size_t r = 0; r < rounds; ++r) {
    for (auto& b : trial) memset(&b, 0, sizeof(b));
    for (auto& kv : classes) {
      Class& c = kv.second;
      if (c.t.empty()) continue;
      const size_t ci = r < c.t.size() ? r : c.t.size() - 1;
      for (size_t i : c.ops)
        for (size_t k = 0; k < c.cands.size(); ++k) trial[i * 4 + k] = c.cands[k][ci];
    }
    h->tuned[shape] = trial;
    std::vector<float> best_ms(n_ops, 1e30f);
    for (int rep = 0; rep < 6; ++rep) {           // first repetition also warms caches for this choice
      rc = run(h, timed);
      if (rc != RTPE_OK) { h->tuned.erase(shape); return rc; }
      if (rep == 0) continue;
      for (size_t i = 0; i < n_ops; ++i) best_ms[i] = ms[i] < best_ms[i] ? ms[i] : best_ms[i];
    }
    for (auto& kv : classes) {
      Class& c = kv.second;
      if (r < c.t.size())
        for (size_t i : c.ops) c.t[r] += best_ms[i];
    }
  }
  std::vector<ConvTile> best(n_ops * 4);
  for (auto& b : best) memset(&b, 0, sizeof(b));
  for (auto& kv : classes) {
    Class& c = kv.second;
    if (c.t.empty()) continue;
    size_t bi = 0;
    double t_max = 0.0;
    for (size_t j = 0; j < c.t.size(); ++j) t_max = c.t[j] > t_max ? c.t[j] : t_max;
    // a class whose ops never ran on their own in these forwards (the second conv of a fused BasicBlock, the stem's conv2
    // inside the fused stem kernel: their time is the head's, theirs reads 0) has nothing to choose from: it stays
    // untuned, and whoever switches the fusion off gets the default launch shape instead of "the first candidate"
    if (t_max <= 0.0) continue;
    for (size_t j = 1; j < c.t.size(); ++j) if (c.t[j] < c.t[bi]) bi = j;
    for (size_t i : c.ops)
      for (size_t k = 0; k < c.cands.size(); ++k) best[i * 4 + k] = c.cands[k][bi];
  }
  h->tuned[shape] = best;
  return RTPE_OK;
}

extern "C" int rtpe_hrnet_autotune(rtpe_hrnet* h, const void* x, int32_t x_dtype, int32_t N, int32_t H, int32_t W,
                                   void* preds, void* refined, int32_t out_dtype, void* workspace,
                                   size_t workspace_bytes, void* stream) {
  return autotune_impl(h, x, x_dtype, nullptr, N, H, W, preds, refined, out_dtype, workspace, workspace_bytes, stream);
}

// the same for a program with a second input (RTPE_OP_AUX_PACK): every timed pass is a rtpe_hrnet_forward_aux
extern "C" int rtpe_hrnet_autotune_aux(rtpe_hrnet* h, const void* x, int32_t x_dtype, const void* aux_nchw_f32, int32_t N,
                                       int32_t H, int32_t W, void* preds, void* refined, int32_t out_dtype,
                                       void* workspace, size_t workspace_bytes, void* stream) {
  RTPE_REQUIRE(aux_nchw_f32 != nullptr, "autotune_aux: the second input is null");
  return autotune_impl(h, x, x_dtype, aux_nchw_f32, N, H, W, preds, refined, out_dtype, workspace, workspace_bytes, stream);
}

// rtpe_hrnet_forward that also records one HIP event per op into `slot` WITHOUT
// synchronising; rtpe_hrnet_read_record(slot) later waits for them and returns the
// per-op times.  Lets bench.py time the ops inside a pipelined timed region.
extern "C" int rtpe_hrnet_forward_record(rtpe_hrnet* h, const void* x, int32_t x_dtype, int32_t N, int32_t H,
                                         int32_t W, void* preds, void* refined, int32_t out_dtype,
                                         void* workspace, size_t workspace_bytes, void* stream, int32_t slot) {
  RTPE_REQUIRE(h != nullptr && slot >= 0 && slot < 64, "forward_record: bad slot");
  FwdCall c = fwd_call(x, x_dtype, N, H, W, preds, refined, out_dtype, workspace, workspace_bytes, stream);
  c.rec = &h->records[slot];
  return run(h, c);
}

extern "C" int rtpe_hrnet_read_record(rtpe_hrnet* h, int32_t slot, float* op_ms, int32_t n_ops) {
  RTPE_REQUIRE(h != nullptr && op_ms != nullptr, "read_record: null argument");
  DeviceGuard guard(h->device);
  auto it = h->records.find(slot);
  RTPE_REQUIRE(it != h->records.end() && it->second.ev.size() == h->ops.size() + 1 && n_ops >= (int)h->ops.size(),
               "read_record: nothing recorded in slot %d", slot);
  RTPE_HIP_CHECK(hipEventSynchronize(it->second.ev.back()));
  return read_op_times(it->second.routes, it->second.ev, op_ms);
}

// ---- tuned launch shapes: export / import (persisted by the caller, e.g. across processes) -------------------
// One record of RTPE_TUNED_INTS int32 per (op, parity class): {nt, waves, th, tw, lds_bytes, kind, grid,
// buf_bytes, n_bufs, n_wslots, mrun}; nt == 0 = not tuned.  Import accepts a record only if it is one of the launch
// shapes conv_enum_tiles offers for that op at this (N, H, W) - a stale or foreign file cannot produce a launch
// the kernels were not built for - and returns RTPE_E_INVALID without changing anything otherwise.
extern "C" int rtpe_hrnet_tuned_ints(const rtpe_hrnet* h, int32_t* count) {
  RTPE_REQUIRE(h != nullptr && count != nullptr, "tuned_ints: null argument");
  *count = (int32_t)(h->ops.size() * 4 * RTPE_TUNED_INTS);
  return RTPE_OK;
}

extern "C" int rtpe_hrnet_export_tuned(const rtpe_hrnet* h, int32_t N, int32_t H, int32_t W, int32_t* out, int32_t n) {
  RTPE_REQUIRE(h != nullptr && out != nullptr, "export_tuned: null argument");
  RTPE_REQUIRE(n >= (int)(h->ops.size() * 4 * RTPE_TUNED_INTS), "export_tuned: buffer too small");
  auto it = h->tuned.find(std::make_tuple((int)N, (int)H, (int)W));
  RTPE_REQUIRE(it != h->tuned.end(), "export_tuned: shape %dx%dx%d has not been tuned", N, H, W);
  for (size_t i = 0; i < it->second.size(); ++i) {
    const ConvTile& t = it->second[i];
    int32_t* r = out + i * RTPE_TUNED_INTS;
    r[0] = t.nt; r[1] = t.waves; r[2] = t.th; r[3] = t.tw; r[4] = (int32_t)t.lds_bytes; r[5] = t.kind;
    r[6] = t.grid; r[7] = t.buf_bytes; r[8] = t.n_bufs; r[9] = t.n_wslots; r[10] = t.mrun;
  }
  return RTPE_OK;
}

extern "C" int rtpe_hrnet_import_tuned(rtpe_hrnet* h, int32_t N, int32_t H, int32_t W, const int32_t* in, int32_t n) {
  RTPE_REQUIRE(h != nullptr && in != nullptr && N > 0 && H >= 32 && W >= 32 && H % 32 == 0 && W % 32 == 0,
               "import_tuned: bad argument");
  const size_t n_ops = h->ops.size();
  RTPE_REQUIRE(n == (int)(n_ops * 4 * RTPE_TUNED_INTS), "import_tuned: %d values for %zu ops", n, n_ops);
  std::vector<ConvTile> tiles(n_ops * 4);
  for (auto& b : tiles) memset(&b, 0, sizeof(b));
  std::vector<ConvTile> cands;
  for (size_t i = 0; i < n_ops; ++i) {
    const OpState& o = h->ops[i];
    const rtpe_op_desc& d = o.d;
    for (int k = 0; k < 4; ++k) {
      const int32_t* r = in + (i * 4 + k) * RTPE_TUNED_INTS;
      if (r[0] == 0) continue;
      RTPE_REQUIRE(k < o.n_geom, "import_tuned: op %zu has no launch shape %d", i, k);
      conv_enum_tiles(o.plan[k], N, conv_pos(h, d, H), conv_pos(h, d, W), &cands);
      bool found = false;
      for (const ConvTile& c : cands) {
        if (c.nt == r[0] && c.waves == r[1] && c.th == r[2] && c.tw == r[3] && (int32_t)c.lds_bytes == r[4] &&
            c.kind == r[5] && c.grid == r[6] && c.buf_bytes == r[7] && c.n_bufs == r[8] && c.n_wslots == r[9] && c.mrun == r[10]) {
          tiles[i * 4 + k] = c;
          found = true;
          break;
        }
      }
      RTPE_REQUIRE(found, "import_tuned: op %zu class %d: not a launch shape of this build", i, k);
    }
  }
  h->tuned[std::make_tuple((int)N, (int)H, (int)W)] = tiles;
  return RTPE_OK;
}
