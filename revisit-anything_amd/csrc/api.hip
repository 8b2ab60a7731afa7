// C-ABI of libsegvlad_hip.so (see include/segvlad.h).  Host-side orchestration only: argument
// checks, host/device pointer staging, scratch sizing and kernel sequencing on the context stream.
// This unit: context, options, staging, guard mode, stage timers, vocabulary, PCA model, pca_apply, normalise, merge_topk / sims /
// minmax, vote.  describe.hip: the describe stage (plan_describe and its staged passes); search.hip: the index and the exact search;
// the searches derived from it (shortlist, match_pairs, excluding, grouped), verify_pairs and sequence_rerank have their entry points next to their kernels.
#include <stdarg.h>
#include <stdlib.h>
#include <string.h>

#include <cmath>
#include <mutex>
#include <utility>

#include <initializer_list>

#include "ctx.h"

int segvlad_ctx::fail(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(err, sizeof(err), fmt, ap);
  va_end(ap);
  return code;
}

bool sv_is_device_ptr(const void* p) {
  hipPointerAttribute_t a;
  memset(&a, 0, sizeof(a));
  hipError_t e = hipPointerGetAttributes(&a, p);
  if (e != hipSuccess) {
    (void)hipGetLastError();  // unregistered host memory reports an error on some runtimes
    return false;
  }
  return a.type == hipMemoryTypeDevice || a.type == hipMemoryTypeManaged || a.type == hipMemoryTypeUnified;
}

void sv_begin(segvlad_ctx* ctx) {
  ctx->stage_used = 0;
  ctx->pending_out.clear();
  ctx->err[0] = 0;
  (void)hipSetDevice(ctx->device);
}

static DevBuf* next_stage(segvlad_ctx* ctx) {
  if (ctx->stage_used >= (int)ctx->stage.size()) {
    ctx->stage.resize(ctx->stage_used + 1);
    ctx->stage.back().tag = "stage";
    ctx->stage.back().guard = ctx->guard;
  }
  return &ctx->stage[ctx->stage_used++];
}

int sv_in(segvlad_ctx* ctx, const void* p, size_t bytes, const void** dev) {
  if (bytes == 0) {
    *dev = p;
    return SEGVLAD_OK;
  }
  if (sv_is_device_ptr(p)) {
    *dev = p;
    return SEGVLAD_OK;
  }
  DevBuf* b = next_stage(ctx);
  SV_HIP(b->reserve(bytes));
  SV_HIP(hipMemcpyAsync(b->p, p, bytes, hipMemcpyHostToDevice, ctx->stream));
  // pageable host memory: hipMemcpyAsync returns after the staging copy, so the caller may reuse p
  *dev = b->p;
  return SEGVLAD_OK;
}

int sv_out(segvlad_ctx* ctx, void* p, size_t bytes, void** dev) {
  if (bytes == 0 || sv_is_device_ptr(p)) {
    *dev = p;
    return SEGVLAD_OK;
  }
  DevBuf* b = next_stage(ctx);
  SV_HIP(b->reserve(bytes));
  ctx->pending_out.push_back({p, b->p, bytes});
  *dev = b->p;
  return SEGVLAD_OK;
}

int sv_finish(segvlad_ctx* ctx) {
  if (!ctx->pending_out.empty()) {
    for (auto& po : ctx->pending_out) SV_HIP(hipMemcpyAsync(po.host, po.dev, po.bytes, hipMemcpyDeviceToHost, ctx->stream));
    SV_HIP(hipStreamSynchronize(ctx->stream));
    ctx->pending_out.clear();
  }
  if (ctx->guard) return sv_guard_check(ctx);
  return SEGVLAD_OK;
}

// ---- guard mode (ctx.h: DevBuf) -----------------------------------------------------------------------------------
static hipError_t guard_fill(void* at) { return hipMemsetD32(reinterpret_cast<hipDeviceptr_t>(at), (int)SV_GUARD_WORD, SV_GUARD_BYTES / 4); }

// number of fence words that no longer hold the poison (0 = intact); < 0: a HIP error
static int guard_words_hit(const void* at) {
  uint32_t h[SV_GUARD_BYTES / 4];
  if (hipMemcpy(h, at, SV_GUARD_BYTES, hipMemcpyDeviceToHost) != hipSuccess) return -1;
  int bad = 0;
  for (uint32_t w : h) bad += (w != SV_GUARD_WORD);
  return bad;
}

hipError_t DevBuf::reserve_guarded(size_t bytes) {
  // every earlier user of this buffer has finished (the fence may move INTO bytes an earlier, larger request used)
  hipError_t e = hipDeviceSynchronize();
  if (e != hipSuccess) return e;
  if (!raw || bytes > cap) {
    // (a trampled fence of the old allocation is caught by the check at the end of the call that trampled it)
    if (raw) {
      e = hipFree(raw);
      if (e != hipSuccess) return e;
      raw = nullptr;
      p = nullptr;
      cap = 0;
    }
    const size_t want = (bytes + 15) & ~(size_t)15;   // exact: no slack to absorb an overrun
    e = hipMalloc(&raw, want + 2 * SV_GUARD_BYTES);
    if (e != hipSuccess) return e;
    p = static_cast<unsigned char*>(raw) + SV_GUARD_BYTES;
    cap = want;
    req = cap;   // (where the back fence of a `fixed` buffer goes, and stays)
    e = guard_fill(raw);
    if (e == hipSuccess) e = guard_fill(static_cast<unsigned char*>(p) + cap);
    if (e != hipSuccess) return e;
  }
  if (!fixed) {
    req = bytes;
    e = guard_fill(static_cast<unsigned char*>(p) + fence_off());
  }
  return e;
}

int sv_fork_side(segvlad_ctx* ctx) {
  if (!ctx->side) {
    SV_HIP(hipStreamCreateWithFlags(&ctx->side, hipStreamNonBlocking));
    SV_HIP(hipEventCreateWithFlags(&ctx->ev_fork, hipEventDisableTiming));
    SV_HIP(hipEventCreateWithFlags(&ctx->ev_join, hipEventDisableTiming));
  }
  SV_HIP(hipEventRecord(ctx->ev_fork, ctx->stream));
  SV_HIP(hipStreamWaitEvent(ctx->side, ctx->ev_fork, 0));
  return SEGVLAD_OK;
}

int sv_join_side(segvlad_ctx* ctx) {
  SV_HIP(hipEventRecord(ctx->ev_join, ctx->side));
  SV_HIP(hipStreamWaitEvent(ctx->stream, ctx->ev_join, 0));
  return SEGVLAD_OK;
}

int sv_guard_check(segvlad_ctx* ctx) {
  if (!ctx->guard) return SEGVLAD_OK;
  SV_HIP(hipDeviceSynchronize());
  if (!ctx->guard_hit[0]) {
    ctx->for_each_buf([&](DevBuf& b) {
      if (!b.raw || ctx->guard_hit[0]) return;
      const int front = guard_words_hit(b.raw), back = guard_words_hit(static_cast<unsigned char*>(b.p) + b.fence_off());
      if (front)
        snprintf(ctx->guard_hit, sizeof(ctx->guard_hit), "%s: %d words written BELOW the buffer", b.tag, front);
      else if (back)
        snprintf(ctx->guard_hit, sizeof(ctx->guard_hit), "%s: %d words written beyond the %zu bytes requested", b.tag, back, b.fixed ? b.cap : b.req);
    });
  }
  if (ctx->guard_hit[0]) return ctx->fail(SEGVLAD_ERR_STATE, "guard: out-of-bounds write, buffer %s", ctx->guard_hit);
  return SEGVLAD_OK;
}

StageTimer* sv_stage_open(segvlad_ctx* c, const char* name, int* slot) {
  if (!c->profiling || c->scope_mute) return nullptr;
  StageTimer* t = &c->timers[name];
  if (t->used * 2 >= (int)t->ev.size()) {
    hipEvent_t a = nullptr, b = nullptr;
    (void)hipEventCreate(&a);
    (void)hipEventCreate(&b);
    t->ev.push_back(a);
    t->ev.push_back(b);
  }
  *slot = t->used++;
  (void)hipEventRecord(t->ev[2 * *slot], c->stream);
  return t;
}

hipError_t sv_max_dyn_lds(const void* fn, size_t bytes) {
  static std::mutex mu;
  static std::map<std::pair<int, const void*>, size_t> done;   // largest size granted so far
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return e;
  std::lock_guard<std::mutex> lk(mu);
  auto it = done.find({dev, fn});
  if (it != done.end() && it->second >= bytes) return hipSuccess;
  e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
  if (e == hipSuccess) done[{dev, fn}] = bytes;
  return e;
}

extern "C" {

int segvlad_version(void) { return 300; }

int segvlad_create(segvlad_ctx** out, int device_id) {
  if (!out) return SEGVLAD_ERR_ARG;
  *out = nullptr;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || device_id < 0 || device_id >= ndev) return SEGVLAD_ERR_HIP;
  if (hipSetDevice(device_id) != hipSuccess) return SEGVLAD_ERR_HIP;
  segvlad_ctx* c = new (std::nothrow) segvlad_ctx();
  if (!c) return SEGVLAD_ERR_NOMEM;
  c->device = device_id;
  // environment defaults of the tuning switches, read once here (segvlad_set_option overrides them later)
  static const char* const env_keys[][2] = {{"SEGVLAD_KNN_FILTER", "knn_filter"},   {"SEGVLAD_F16_CFG", "f16_cfg"},
                                            {"SEGVLAD_F16_GM", "f16_gm"},           {"SEGVLAD_X3_TILE", "x3_tile"},
                                            {"SEGVLAD_X3_GM", "x3_gm"},             {"SEGVLAD_SEARCH_STATS", "search_stats"},
                                            {"SEGVLAD_ASSIGN_NARROW", "assign_narrow"}, {"SEGVLAD_DEBUG_SEARCH", "debug_search"},
                                            {"SEGVLAD_AGG_KPB", "agg_kpb"},
                                            {"SEGVLAD_KNN_HEURISTIC", "knn_heuristic"}, {"SEGVLAD_PCA_PATH", "pca_path"},
                                            {"SEGVLAD_COVER_ROWS", "cover_rows"}};
  for (auto& kv : env_keys)
    if (const char* v = getenv(kv[0])) (void)segvlad_set_option(c, kv[1], v);
#define SV_TAG_P(n) c->n.tag = #n; c->n.fixed = true;
#define SV_TAG_S(n) c->n.tag = #n;
  SV_PERSISTENT_BUFS(SV_TAG_P)
  SV_SCRATCH_BUFS(SV_TAG_S)
#undef SV_TAG_P
#undef SV_TAG_S
  if (const char* v = getenv("SEGVLAD_GUARD")) {
    if (v[0] && v[0] != '0') {
      c->guard = true;
      c->for_each_buf([](DevBuf& b) { b.guard = true; });
    }
  }
  if (const char* v = getenv("SEGVLAD_RCCL_LIB")) snprintf(sv_rccl_lib_override, sizeof(sv_rccl_lib_override), "%s", v);
  if (getenv("SEGVLAD_KNN_FP32")) (void)segvlad_set_option(c, "knn_filter", "fp32");
  if (getenv("SEGVLAD_PCA_FP32")) (void)segvlad_set_option(c, "pca_arith", "fp32");
  c->err[0] = 0;
  *out = c;
  return SEGVLAD_OK;
}

int segvlad_set_option(segvlad_ctx* ctx, const char* key, const char* value) {
  if (!ctx) return SEGVLAD_ERR_ARG;
  if (!key || !value) return ctx->fail(SEGVLAD_ERR_ARG, "set_option: null key/value");
  SvOptions& o = ctx->opt;
  auto as_int = [&](int* dst) -> int {
    char* end = nullptr;
    const long v = strtol(value, &end, 10);
    if (end == value || *end) return ctx->fail(SEGVLAD_ERR_ARG, "set_option(%s): '%s' is not an integer", key, value);
    *dst = (int)v;
    return SEGVLAD_OK;
  };
  if (!strcmp(key, "knn_filter")) {
    if (!strcmp(value, "auto")) o.knn_filter = 0;
    else if (!strcmp(value, "f16")) o.knn_filter = 1;
    else if (!strcmp(value, "bf16x3")) o.knn_filter = 2;
    else if (!strcmp(value, "fp32")) o.knn_filter = 3;
    else return ctx->fail(SEGVLAD_ERR_ARG, "set_option(knn_filter): want auto|f16|bf16x3|fp32, got '%s'", value);
    return SEGVLAD_OK;
  }
  if (!strcmp(key, "pca_arith")) {
    if (!strcmp(value, "auto") || !strcmp(value, "f16x3")) o.pca_fp32 = 0;
    else if (!strcmp(value, "fp32")) o.pca_fp32 = 1;
    else return ctx->fail(SEGVLAD_ERR_ARG, "set_option(pca_arith): want auto|f16x3|fp32, got '%s'", value);
    return SEGVLAD_OK;
  }
  if (!strcmp(key, "pca_path")) {
    if (!strcmp(value, "auto")) o.pca_path = 0;
    else if (!strcmp(value, "planes")) o.pca_path = 1;
    else if (!strcmp(value, "project")) o.pca_path = 2;
    else return ctx->fail(SEGVLAD_ERR_ARG, "set_option(pca_path): want auto|planes|project, got '%s'", value);
    return SEGVLAD_OK;
  }
  if (!strcmp(key, "vlad_assign")) {   // hard | soft:<T> | soft_pooled:<T>, T a decimal fp32, finite, > 0 (include/segvlad.h); a refusal
                                       // changes nothing
    if (!strcmp(value, "hard")) {
      o.vlad_soft_temp = 0.f, o.vlad_soft_pooled = 0;
      return SEGVLAD_OK;
    }
    const int pooled = !strncmp(value, "soft_pooled:", 12);
    if (pooled || !strncmp(value, "soft:", 5)) {
      const char* t = value + (pooled ? 12 : 5);
      bool decimal = *t != 0 && (*t == '.' || (*t >= '0' && *t <= '9'));
      for (const char* c = t; *c && decimal; ++c) decimal = strchr("0123456789.eE+-", *c) != nullptr;
      char* end = nullptr;
      const float temp = decimal ? strtof(t, &end) : 0.f;
      if (decimal && end != t && *end == 0 && std::isfinite(temp) && temp > 0.f) {
        o.vlad_soft_temp = temp, o.vlad_soft_pooled = pooled;
        return SEGVLAD_OK;
      }
    }
    return ctx->fail(SEGVLAD_ERR_ARG, "set_option(vlad_assign): want hard|soft:<T>|soft_pooled:<T> with a finite decimal T > 0, got '%s'", value);
  }
  if (!strcmp(key, "vlad_burst")) {   // off | <a>:<b>:<p>, three decimal fp32 with 0 <= a <= 64, -8 <= b <= 16, 0 <= p <= 2
                                      // (include/segvlad.h); vlad_assign's strictness, a refusal changes nothing
    if (!strcmp(value, "off")) {
      o.vlad_burst = 0, o.burst_a = o.burst_b = o.burst_p = 0.f;
      return SEGVLAD_OK;
    }
    static const float lo[3] = {0.f, -8.f, 0.f}, hi[3] = {64.f, 16.f, 2.f};
    float v[3] = {0.f, 0.f, 0.f};
    const char* t = value;
    bool ok = true;
    for (int f = 0; f < 3 && ok; ++f) {
      const char* stop = f < 2 ? strchr(t, ':') : t + strlen(t);   // (a fourth field leaves a ':' inside the third: not a decimal)
      ok = stop != nullptr && stop != t && (*t == '.' || *t == '-' || (*t >= '0' && *t <= '9'));
      for (const char* c = t; ok && c < stop; ++c) ok = strchr("0123456789.eE+-", *c) != nullptr;
      if (!ok) break;
      char* end = nullptr;
      v[f] = strtof(t, &end);
      ok = end == stop && std::isfinite(v[f]) && v[f] >= lo[f] && v[f] <= hi[f];
      t = stop + 1;
    }
    if (ok) {
      o.vlad_burst = 1, o.burst_a = v[0], o.burst_b = v[1], o.burst_p = v[2];
      return SEGVLAD_OK;
    }
    return ctx->fail(SEGVLAD_ERR_ARG, "set_option(vlad_burst): want off|<a>:<b>:<p>, finite decimals with 0 <= a <= 64, -8 <= b <= 16, "
                                      "0 <= p <= 2, got '%s'", value);
  }
  if (!strcmp(key, "vlad_burst_scope")) {   // image | segment (include/segvlad.h); stored whatever vlad_burst holds, read only while it is on
    if (!strcmp(value, "image")) return o.burst_segment = 0, SEGVLAD_OK;
    if (!strcmp(value, "segment")) return o.burst_segment = 1, SEGVLAD_OK;
    return ctx->fail(SEGVLAD_ERR_ARG, "set_option(vlad_burst_scope): want image|segment, got '%s'", value);
  }
  // Switches that select one of the fp16 filter's kernels (csrc/segvlad_dev.h): only the values that name a kernel the library
  // holds are accepted -- the measured-and-not-kept variants are gone from the tree (DESIGN.md 4 / 7 keep their numbers); the
  // development build (-DSEGVLAD_ABLATIONS: lib/libsegvlad_hip_abl.so) adds the probes of the batch kernel.
  auto as_dev = [&](int* dst, std::initializer_list<int> product_values, std::initializer_list<int> probe_values = {}) -> int {
    int v = *dst;
    SV_TRY(as_int(&v));
    bool ok = false;
    for (int a : product_values) ok = ok || a == v;
#ifdef SEGVLAD_ABLATIONS
    for (int a : probe_values) ok = ok || a == v;
#else
    (void)probe_values;
#endif
    if (!ok)
      return ctx->fail(SEGVLAD_ERR_ARG, "set_option(%s=%d): a development switch -- this library holds the default kernels only "
                       "(SEGVLAD_BUILD_ABLATIONS=1 builds lib/libsegvlad_hip_abl.so with the probes of csrc/segvlad_dev.h)", key, v);
    *dst = v;
    return SEGVLAD_OK;
  };
  if (!strcmp(key, "f16_cfg")) return as_dev(&o.f16_cfg, {-1, 250, 300, 62, 63}, {93, 94, 95});
  if (!strcmp(key, "f16_gm")) return as_int(&o.f16_gm);
  if (!strcmp(key, "f16_walk")) return as_int(&o.f16_walk);
  if (!strcmp(key, "f16_deep_cfg")) return as_dev(&o.f16_deep_cfg, {-1, 4, 5});
  if (!strcmp(key, "f16_buf")) return as_dev(&o.f16_buf, {-1, 0});
  if (!strcmp(key, "tnk_gram")) return as_int(&o.tnk_gram);
  if (!strcmp(key, "tnk_fork")) return as_int(&o.tnk_fork);
  if (!strcmp(key, "x3_tile")) return as_int(&o.x3_tile);
  if (!strcmp(key, "x3_gm")) return as_int(&o.x3_gm);
  if (!strcmp(key, "search_stats")) return as_int(&o.search_stats);
  if (!strcmp(key, "knn_heuristic")) return as_int(&o.knn_heuristic);
  if (!strcmp(key, "assign_narrow")) return as_int(&o.assign_narrow);
  if (!strcmp(key, "agg_kpb")) return as_int(&o.agg_kpb);
  if (!strcmp(key, "pj_nw")) return as_int(&o.pj_nw);
  if (!strcmp(key, "pj_f16")) return as_int(&o.pj_f16);
  if (!strcmp(key, "cover_rows")) return as_int(&o.cover_rows);
  if (!strcmp(key, "pj_planes")) return as_int(&o.pj_planes);
  if (!strcmp(key, "small_plan")) return as_int(&o.small_plan);
  if (!strcmp(key, "small_tail")) return as_int(&o.small_tail);
  if (!strcmp(key, "small_head")) return as_int(&o.small_head);
  if (!strcmp(key, "batch_l0_f16")) return as_int(&o.batch_l0_f16);
  if (!strcmp(key, "level_carry")) return as_int(&o.level_carry);
  if (!strcmp(key, "f16_persist_wgs")) return as_int(&o.f16_persist_wgs);
  if (!strcmp(key, "debug_small_tail")) return as_int(&o.debug_small_tail);
  if (!strcmp(key, "refine_group")) return as_int(&o.refine_group);
  if (!strcmp(key, "query_group")) return as_int(&o.query_group);
  if (!strcmp(key, "group_fetch")) return as_int(&o.group_fetch);
  if (!strcmp(key, "debug_search")) return as_int(&o.debug_search);
  if (!strcmp(key, "debug_fail_search")) return as_int(&o.debug_fail_search);
  if (!strcmp(key, "guard_undersize")) {
    // tests of the guard itself: "<buffer tag>:<bytes>" puts that scratch buffer's back fence <bytes> EARLY from its next
    // reserve() on, so that a correct kernel writes into the fence (guard mode only; "" / "none" clears every shrink)
    if (!ctx->guard) return ctx->fail(SEGVLAD_ERR_STATE, "set_option(guard_undersize): the context was not created under SEGVLAD_GUARD=1");
    const char* colon = strchr(value, ':');
    bool found = false;
    ctx->for_each_buf([&](DevBuf& b) {
      if (!colon) b.shrink = 0;
      else if (strlen(b.tag) == (size_t)(colon - value) && !strncmp(b.tag, value, (size_t)(colon - value))) {
        b.shrink = atoi(colon + 1);
        found = true;
      }
    });
    if (colon && !found) return ctx->fail(SEGVLAD_ERR_ARG, "set_option(guard_undersize): no buffer named like '%s'", value);
    return SEGVLAD_OK;
  }
  return ctx->fail(SEGVLAD_ERR_ARG, "set_option: unknown key '%s'", key);
}

int segvlad_destroy(segvlad_ctx* ctx) {
  if (!ctx) return SEGVLAD_OK;
  (void)hipSetDevice(ctx->device);
  (void)hipStreamSynchronize(ctx->stream);
  sv_comm_release(ctx);
  if (ctx->side) {
    (void)hipStreamSynchronize(ctx->side);
    (void)hipStreamDestroy(ctx->side);
    (void)hipEventDestroy(ctx->ev_fork);
    (void)hipEventDestroy(ctx->ev_join);
  }
  if (ctx->h_pin) {
    (void)hipHostFree(ctx->h_pin);
    (void)hipEventDestroy(ctx->ev_scalars);
  }
  if (ctx->h_desc) (void)hipHostFree(ctx->h_desc);
  if (ctx->ev_desc) (void)hipEventDestroy(ctx->ev_desc);
  ctx->for_each_buf([](DevBuf& b) { b.release(); });
  for (auto& kv : ctx->timers)
    for (hipEvent_t e : kv.second.ev)
      if (e) (void)hipEventDestroy(e);
  delete ctx;
  return SEGVLAD_OK;
}

const char* segvlad_last_error(const segvlad_ctx* ctx) { return ctx ? ctx->err : "null context"; }

int segvlad_set_stream(segvlad_ctx* ctx, void* hip_stream) {
  if (!ctx) return SEGVLAD_ERR_ARG;
  ctx->stream = reinterpret_cast<hipStream_t>(hip_stream);
  return SEGVLAD_OK;
}

int segvlad_synchronize(segvlad_ctx* ctx) {
  CHECK_CTX();
  SV_HIP(hipStreamSynchronize(ctx->stream));
  return sv_guard_check(ctx);   // (guard mode only: SEGVLAD_ERR_STATE if a buffer's fence has been written)
}

int segvlad_set_profiling(segvlad_ctx* ctx, int on) {
  if (!ctx) return SEGVLAD_ERR_ARG;
  ctx->profiling = on != 0;
  return SEGVLAD_OK;
}

int segvlad_profile_reset(segvlad_ctx* ctx) {
  if (!ctx) return SEGVLAD_ERR_ARG;
  for (auto& kv : ctx->timers) {
    kv.second.used = 0;
    kv.second.launches = 0;
  }
  return SEGVLAD_OK;
}

int segvlad_stage_ms(segvlad_ctx* ctx, const char* stage, float* ms_out, int* launches_out) {
  CHECK_CTX();
  if (!stage || !ms_out) return ctx->fail(SEGVLAD_ERR_ARG, "stage_ms: null argument");
  auto it = ctx->timers.find(stage);
  if (it == ctx->timers.end() || it->second.used == 0)
    return ctx->fail(SEGVLAD_ERR_STATE, "stage '%s' has not run with profiling on", stage);
  StageTimer& t = it->second;
  double total = 0.0;
  for (int i = 0; i < t.used; ++i) {
    SV_HIP(hipEventSynchronize(t.ev[2 * i + 1]));
    float ms = 0.f;
    SV_HIP(hipEventElapsedTime(&ms, t.ev[2 * i], t.ev[2 * i + 1]));
    total += ms;
  }
  *ms_out = (float)total;
  if (launches_out) *launches_out = t.launches;
  return SEGVLAD_OK;
}

// ---- vocabulary ----------------------------------------------------------------------------------
int segvlad_set_vocab(segvlad_ctx* ctx, const float* C, int K, int D) {
  CHECK_CTX();
  if (!C || K <= 0 || D <= 0) return ctx->fail(SEGVLAD_ERR_ARG, "set_vocab: need C, K>0, D>0");
  if (D % 4) return ctx->fail(SEGVLAD_ERR_ARG, "set_vocab: D=%d must be a multiple of 4", D);
  if (K > 128) return ctx->fail(SEGVLAD_ERR_LIMIT, "set_vocab: K=%d > 128 clusters is not supported by this build", K);
  int Kpad = (K <= 32) ? 32 : (K <= 64) ? 64 : 128;
  const size_t bytes = (size_t)K * D * sizeof(float);
  SV_HIP(ctx->vocab.reserve(bytes));
  if (sv_is_device_ptr(C))
    SV_HIP(hipMemcpyAsync(ctx->vocab.p, C, bytes, hipMemcpyDeviceToDevice, ctx->stream));
  else
    SV_HIP(hipMemcpyAsync(ctx->vocab.p, C, bytes, hipMemcpyHostToDevice, ctx->stream));
  ctx->K = K;
  ctx->D = D;
  ctx->Kpad = Kpad;
  SV_TRY(sv_launch_vocab_prepare(ctx));
  // largest centre component: bounds the token residuals x^ - C_k whose fp16 planes the "project" form builds (plan_describe)
  SV_TRY(sv_maxabs(ctx, ctx->vocab.as<float>(), (int64_t)K * D, &ctx->vocab_maxabs));
  // largest centre norm: ||x^ - C_k|| <= 1 + max ||C_k||, the bound behind the fp16 split of the PROJECTED residuals (the P-space
  // sums of the "project" form on the 16-bit pipe)
  {
    float n2 = 0.f;
    SV_HIP(ctx->s_qnorm.reserve((size_t)K * sizeof(float)));
    SV_TRY(sv_launch_row_sumsq(ctx, ctx->vocab.as<float>(), K, D, ctx->s_qnorm.as<float>()));
    SV_TRY(sv_row_norm_max(ctx, ctx->s_qnorm.as<float>(), K, &n2));
    ctx->vocab_norm_max = std::sqrt(n2 > 0.f ? n2 : 0.f);
  }
  return sv_finish(ctx);
}

// ---- PCA ------------------------------------------------------------------------------------------------
__global__ void pca_scale_kernel(const float* var, int P, int whiten, float* scale) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j < P) scale[j] = whiten ? (float)(1.0 / sqrt((double)var[j])) : 1.f;
}

int segvlad_pca_set(segvlad_ctx* ctx, const float* mean, const float* comps, const float* expl_var, int P, int KD,
                    int whiten) {
  CHECK_CTX();
  if (!comps || P <= 0 || KD <= 0) return ctx->fail(SEGVLAD_ERR_ARG, "pca_set: need comps, P>0, KD>0");
  if (whiten && !expl_var) return ctx->fail(SEGVLAD_ERR_ARG, "pca_set: whiten needs explained_variance");
  SV_HIP(ctx->pca_comps.reserve((size_t)P * KD * sizeof(float)));
  SV_HIP(ctx->pca_mean.reserve((size_t)KD * sizeof(float)));
  SV_HIP(ctx->pca_scale.reserve((size_t)P * sizeof(float)));
  SV_HIP(hipMemcpyAsync(ctx->pca_comps.p, comps, (size_t)P * KD * sizeof(float), hipMemcpyDefault, ctx->stream));
  if (mean)
    SV_HIP(hipMemcpyAsync(ctx->pca_mean.p, mean, (size_t)KD * sizeof(float), hipMemcpyDefault, ctx->stream));
  else
    SV_HIP(hipMemsetAsync(ctx->pca_mean.p, 0, (size_t)KD * sizeof(float), ctx->stream));
  const void* dvar = nullptr;
  if (whiten) SV_TRY(sv_in(ctx, expl_var, (size_t)P * sizeof(float), &dvar));
  hipLaunchKernelGGL(pca_scale_kernel, dim3((P + 255) / 256), dim3(256), 0, ctx->stream, (const float*)dvar, P, whiten,
                     ctx->pca_scale.as<float>());
  SV_HIP(hipGetLastError());
  ctx->P = P;
  ctx->KD = KD;
  ctx->whiten = whiten;
  ctx->pca_cproj_valid = false;
  ctx->pca_w_scale = 0.f;
  if (KD % 32 == 0) {  // fp16 two-term split of the components for the 16-bit MFMA projection
    float wmax = 0.f, mmax = 0.f;
    SV_TRY(sv_maxabs(ctx, ctx->pca_comps.as<float>(), (int64_t)P * KD, &wmax));
    SV_TRY(sv_maxabs(ctx, ctx->pca_mean.as<float>(), KD, &mmax));
    if (wmax > 0.f && std::isfinite(wmax)) {
      ctx->pca_w_scale = sv_fp16_scale(wmax);
      ctx->pca_mean_maxabs = mmax;
      SV_HIP(ctx->pca_w1.reserve((size_t)sv_x3_rows(P) * KD * 2));   // blocked planes, rows padded to whole tiles
      SV_HIP(ctx->pca_w2.reserve((size_t)sv_x3_rows(P) * KD * 2));
      SV_TRY(sv_launch_split_f16x2(ctx, ctx->pca_comps.as<float>(), P, KD, nullptr, ctx->pca_w_scale, ctx->pca_w1.as<uint16_t>(),
                                   ctx->pca_w2.as<uint16_t>()));
    }
  }
  SV_HIP(hipStreamSynchronize(ctx->stream));
  return sv_finish(ctx);
}

int segvlad_pca_apply(segvlad_ctx* ctx, const float* X, int n, float* Y, int l2norm) {
  CHECK_CTX();
  if (ctx->P == 0) return ctx->fail(SEGVLAD_ERR_STATE, "pca_apply: call segvlad_pca_set first");
  if (n < 0) return ctx->fail(SEGVLAD_ERR_ARG, "pca_apply: n<0");
  if (n == 0) return SEGVLAD_OK;
  if (!X || !Y) return ctx->fail(SEGVLAD_ERR_ARG, "pca_apply: null pointer");
  const void* dx;
  void* dy;
  SV_TRY(sv_in(ctx, X, (size_t)n * ctx->KD * sizeof(float), &dx));
  SV_TRY(sv_out(ctx, Y, (size_t)n * ctx->P * sizeof(float), &dy));
  const bool x3 = ctx->pca_w_scale > 0.f && !ctx->opt.pca_fp32;
  // the split kernel loads 16-byte pieces.  Refused rather than staged as segvlad_search_shortlist stages its queries: X can be
  // the PCA fit's resident matrix (tens of GB), a copy of which the context cannot promise; the fp32 kernel takes any pointer.
  if (x3 && (reinterpret_cast<uintptr_t>(dx) & 15) != 0)
    return ctx->fail(SEGVLAD_ERR_ARG, "pca_apply: X must be 16-byte aligned for the fp16x3 projection (or set pca_arith=fp32)");
  float xscale = 1.f;
  if (x3) {  // ONE scale for the batch, so that |x - mean| * s < 2^15: no fp16 overflow; rows down to 2^-12 of the batch maximum keep
             // both fp16 terms normal (include/segvlad.h).  The maximum is taken over the FINITE entries: a NaN / Inf row gives a
             // non-finite row of Y and must not cost the other rows their scale.
    float xmax = 0.f;
    SV_TRY(sv_maxabs(ctx, (const float*)dx, (int64_t)n * ctx->KD, &xmax, /*finite_only=*/true));
    const float bound = xmax + ctx->pca_mean_maxabs;
    if (bound > 0.f && std::isfinite(bound)) xscale = sv_fp16_scale(bound);
    SV_HIP(ctx->s_xh1.reserve((size_t)sv_x3_rows(n) * ctx->KD * 2));
    SV_HIP(ctx->s_xh2.reserve((size_t)sv_x3_rows(n) * ctx->KD * 2));
  }
  {
    StageScope sc(ctx, "pca");
    if (x3) {
      SV_TRY(sv_launch_split_f16x2(ctx, (const float*)dx, n, ctx->KD, ctx->pca_mean.as<float>(), xscale, ctx->s_xh1.as<uint16_t>(),
                                   ctx->s_xh2.as<uint16_t>()));
      SV_TRY(sv_launch_gemm_f16x3(ctx, ctx->s_xh1.as<uint16_t>(), ctx->s_xh2.as<uint16_t>(), ctx->pca_w1.as<uint16_t>(),
                                  ctx->pca_w2.as<uint16_t>(), n, ctx->P, ctx->KD, 1.f / (xscale * ctx->pca_w_scale),
                                  ctx->pca_scale.as<float>(), (float*)dy));
      sc.count(3);
    } else {
      SV_TRY(sv_launch_gemm_nt(ctx, 0, (const float*)dx, ctx->pca_comps.as<float>(), (float*)dy, n, ctx->P, ctx->KD, ctx->P,
                               ctx->pca_mean.as<float>(), ctx->pca_scale.as<float>(), nullptr, nullptr));
      sc.count();
    }
    if (l2norm) {
      SV_TRY(sv_launch_normalize_rows(ctx, (const float*)dy, n, ctx->P, (float*)dy));
      sc.count();
    }
  }
  return sv_finish(ctx);
}

int segvlad_normalize_rows(segvlad_ctx* ctx, const float* X, int n, int d, float* Y) {
  CHECK_CTX();
  if (n < 0 || d <= 0) return ctx->fail(SEGVLAD_ERR_ARG, "normalize_rows: bad shape");
  if (n == 0) return SEGVLAD_OK;
  if (!X || !Y) return ctx->fail(SEGVLAD_ERR_ARG, "normalize_rows: null pointer");
  const void* dx;
  void* dy;
  SV_TRY(sv_in(ctx, X, (size_t)n * d * sizeof(float), &dx));
  SV_TRY(sv_out(ctx, Y, (size_t)n * d * sizeof(float), &dy));
  SV_TRY(sv_launch_normalize_rows(ctx, (const float*)dx, n, d, (float*)dy));
  return sv_finish(ctx);
}

int segvlad_merge_topk(segvlad_ctx* ctx, const float* d2_parts, const int64_t* idx_parts, int nq, int parts, int k,
                       float* d2_out, int64_t* idx_out) {
  CHECK_CTX();
  if (nq < 0 || parts < 1 || k < 1) return ctx->fail(SEGVLAD_ERR_ARG, "merge_topk: bad shape");
  if (nq == 0) return SEGVLAD_OK;
  if (!d2_parts || !idx_parts || !d2_out || !idx_out) return ctx->fail(SEGVLAD_ERR_ARG, "merge_topk: null pointer");
  const int cand = parts * k;
  const void *dd, *di;
  void *od, *oi;
  SV_TRY(sv_in(ctx, d2_parts, (size_t)nq * cand * 4, &dd));
  SV_TRY(sv_in(ctx, idx_parts, (size_t)nq * cand * 8, &di));
  SV_TRY(sv_out(ctx, d2_out, (size_t)nq * k * 4, &od));
  SV_TRY(sv_out(ctx, idx_out, (size_t)nq * k * 8, &oi));
  SV_TRY(sv_launch_merge_topk(ctx, (const float*)dd, (const int64_t*)di, nq, cand, k, (float*)od, (int64_t*)oi));
  return sv_finish(ctx);
}

int segvlad_sims_from_d2(segvlad_ctx* ctx, const float* d2, const int64_t* idx, int nq, int k_in, int k_keep,
                         float* sims_out, int64_t* idx_out) {
  CHECK_CTX();
  if (nq < 0 || k_in < 1 || k_keep < 1 || k_keep > k_in) return ctx->fail(SEGVLAD_ERR_ARG, "sims_from_d2: bad shape");
  if (nq == 0) return SEGVLAD_OK;
  if (!d2 || !idx || !sims_out || !idx_out) return ctx->fail(SEGVLAD_ERR_ARG, "sims_from_d2: null pointer");
  const void *dd, *di;
  void *os, *oi;
  SV_TRY(sv_in(ctx, d2, (size_t)nq * k_in * 4, &dd));
  SV_TRY(sv_in(ctx, idx, (size_t)nq * k_in * 8, &di));
  SV_TRY(sv_out(ctx, sims_out, (size_t)nq * k_keep * 4, &os));
  SV_TRY(sv_out(ctx, idx_out, (size_t)nq * k_keep * 8, &oi));
  SV_TRY(sv_launch_sims(ctx, (const float*)dd, (const int64_t*)di, nq, k_in, k_keep, (float*)os, (int64_t*)oi));
  return sv_finish(ctx);
}

int segvlad_minmax(segvlad_ctx* ctx, const float* sims, int64_t count, float* minmax_out) {
  CHECK_CTX();
  if (count < 0 || !minmax_out) return ctx->fail(SEGVLAD_ERR_ARG, "minmax: bad arguments");
  const void* ds = sims;
  void* dout;
  if (count > 0) {
    if (!sims) return ctx->fail(SEGVLAD_ERR_ARG, "minmax: null sims");
    SV_TRY(sv_in(ctx, sims, (size_t)count * 4, &ds));
  }
  SV_TRY(sv_out(ctx, minmax_out, 2 * sizeof(float), &dout));
  SV_TRY(sv_launch_minmax(ctx, (const float*)ds, count, (float*)dout));
  return sv_finish(ctx);
}

}  // extern "C"

// The argument checks and the staging of segvlad_vote, shared with segvlad_vote_global (comm.hip): on return the operands
// are on the device and the query-image offsets are on their way to ctx->s_voteoff; v->mm is the two-float extrema slot
// behind them.  n_img == 0 returns SEGVLAD_OK with nothing staged.  mode is decoded here (v->base); with SEGVLAD_VOTE_UNIQUE_REF
// and / or a per-image cap in its bits 8..15 the blanked copy of idx is made behind the staging -- the one-to-one pass first, into
// ctx->s_vote_uniq, then the cap over that copy into ctx->s_vote_cap -- and v->di names the last copy.
int sv_vote_prepare(segvlad_ctx* ctx, const int64_t* idx, const float* sims, const int32_t* img_of_seg, int64_t n_ref_seg,
                    const int32_t* qseg_offsets, int n_img, int k, int n_top, int mode, int32_t* pred_out, double* score_out,
                    SvVote* v) {
  *v = SvVote{};
  if (n_img < 0 || k < 1 || n_top < 1) return ctx->fail(SEGVLAD_ERR_ARG, "vote: bad shape");
  const int base = mode & 0x7f, cap = (mode >> 8) & 0xff;
  const bool unique = (mode & SEGVLAD_VOTE_UNIQUE_REF) != 0;
  if ((mode >> 16) != 0 || (base != SEGVLAD_VOTE_WT_BORDA_IM && base != SEGVLAD_VOTE_COUNT))
    return ctx->fail(SEGVLAD_ERR_ARG, "vote: unknown mode %d", mode);
  v->base = base;
  if (n_img == 0) return SEGVLAD_OK;
  if (!idx || !qseg_offsets || !pred_out) return ctx->fail(SEGVLAD_ERR_ARG, "vote: null pointer");
  if (base == SEGVLAD_VOTE_WT_BORDA_IM && !sims) return ctx->fail(SEGVLAD_ERR_ARG, "vote: weighted mode needs sims");
  if (sv_is_device_ptr(qseg_offsets)) return ctx->fail(SEGVLAD_ERR_ARG, "vote: qseg_offsets must be host memory");
  const int nq = qseg_offsets[n_img];
  int64_t n_ref = ctx->db_n;
  const void* dimg = nullptr;
  if (img_of_seg) {
    if (n_ref_seg <= 0) return ctx->fail(SEGVLAD_ERR_ARG, "vote: an explicit img_of_seg map needs n_ref_seg > 0");
    n_ref = n_ref_seg;
    SV_TRY(sv_in(ctx, img_of_seg, (size_t)n_ref * 4, &dimg));
  } else {
    if (!ctx->db_has_img) return ctx->fail(SEGVLAD_ERR_STATE, "vote: no img_of_seg map: give it to segvlad_db_add");
    dimg = ctx->db_img.p;
  }
  const void *di, *ds = nullptr;
  void *op, *os = nullptr;
  SV_TRY(sv_in(ctx, idx, (size_t)nq * k * 8, &di));
  if (sims) SV_TRY(sv_in(ctx, sims, (size_t)nq * k * 4, &ds));
  SV_TRY(sv_out(ctx, pred_out, (size_t)n_img * n_top * 4, &op));
  if (score_out) SV_TRY(sv_out(ctx, score_out, (size_t)n_img * n_top * 8, &os));
  SV_HIP(ctx->s_voteoff.reserve((size_t)(n_img + 1) * 4 + 32));
  SV_HIP(hipMemcpyAsync(ctx->s_voteoff.p, qseg_offsets, (size_t)(n_img + 1) * 4, hipMemcpyHostToDevice, ctx->stream));
  if (unique && nq > 0) {
    SV_HIP(ctx->s_vote_uniq.reserve((size_t)nq * k * 8));
    StageScope sc(ctx, "vote");
    int launches = 0;
    SV_TRY(sv_launch_vote_unique(ctx, (const int64_t*)di, (const float*)ds, n_ref, ctx->s_voteoff.as<int32_t>(), qseg_offsets, n_img, k,
                                 ctx->s_vote_uniq.as<int64_t>(), &launches));
    sc.count(launches);
    di = ctx->s_vote_uniq.p;
  }
  if (cap > 0 && nq > 0) {
    SV_HIP(ctx->s_vote_cap.reserve((size_t)nq * k * 8));
    StageScope sc(ctx, "vote");
    SV_TRY(sv_launch_vote_cap(ctx, (const int64_t*)di, (const int32_t*)dimg, n_ref, nq, k, cap, ctx->s_vote_cap.as<int64_t>()));
    sc.count();
    di = ctx->s_vote_cap.p;
  }
  v->di = di;
  v->ds = ds;
  v->dimg = dimg;
  v->n_ref = n_ref;
  v->op = op;
  v->os = os;
  v->mm = reinterpret_cast<float*>(ctx->s_voteoff.as<char>() + (((size_t)(n_img + 1) * 4 + 7) & ~7ull));
  v->nq = nq;
  return SEGVLAD_OK;
}

extern "C" {

int segvlad_vote(segvlad_ctx* ctx, const int64_t* idx, const float* sims, const int32_t* img_of_seg,
                 int64_t n_ref_seg, const int32_t* qseg_offsets, int n_img, int k, float smin, float smax, int n_top, int mode,
                 int32_t* pred_out, double* score_out) {
  CHECK_CTX();
  SvVote v;
  SV_TRY(sv_vote_prepare(ctx, idx, sims, img_of_seg, n_ref_seg, qseg_offsets, n_img, k, n_top, mode, pred_out, score_out, &v));
  if (n_img == 0) return SEGVLAD_OK;
  StageScope sc(ctx, "vote");
  if (v.base == SEGVLAD_VOTE_WT_BORDA_IM) {
    if (std::isnan(smin) || std::isnan(smax)) {
      SV_TRY(sv_launch_minmax(ctx, (const float*)v.ds, (int64_t)v.nq * k, v.mm));
      sc.count(3);
    } else {
      const float h[2] = {smin, smax};
      SV_HIP(hipMemcpyAsync(v.mm, h, sizeof(h), hipMemcpyHostToDevice, ctx->stream));
      SV_HIP(hipStreamSynchronize(ctx->stream));
    }
  }
  SV_TRY(sv_launch_vote(ctx, (const int64_t*)v.di, (const float*)v.ds, (const int32_t*)v.dimg, v.n_ref, ctx->s_voteoff.as<int32_t>(),
                        qseg_offsets, n_img, k, v.mm, n_top, v.base, (int32_t*)v.op, (double*)v.os));
  sc.count();
  return sv_finish(ctx);
}

}  // extern "C"
