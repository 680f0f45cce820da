// cvr_options.cpp — cvr_set_option / cvr_get_option (include/cvr.h): one table,
// one row per key, read by both.
#include <hip/hip_runtime.h>

#include <climits>
#include <cstdio>
#include <cstring>

#include "cvr_host.h"

using namespace cvr;

namespace {

struct Option {
  const char* key;
  int Ctx::*field;                          // where a plain option lives (null: `get` computes it)
  int (*get)(const Ctx*);
  int lo, hi;                               // accepted values; lo > hi: read-only
  bool (*ok)(int);                          // null, or what else an in-range value must satisfy
  const char* expect;                       // the error reads "<key> must be <expect>"; null: from lo, hi
  // null, or what an accepted value does besides being stored.  Runs before the
  // store (`value` may be normalised); a failure leaves the option unchanged.
  cvr_status (*apply)(Ctx*, int& value);
};

constexpr int kNone = INT_MIN, kAny = INT_MAX;   // open ends of a range

void invalidate_orders(Ctx* c) {
  for (auto& o : c->oslot) o.valid = 0;
}
cvr_status apply_orders(Ctx* c, int&) {
  invalidate_orders(c);
  return CVR_OK;
}
cvr_status apply_flag(Ctx*, int& value) {
  value = value != 0;
  return CVR_OK;
}

const Option kOptions[] = {
    {"batch", &Ctx::batch, nullptr, 0, 4, [](int v) { return v != 1 && v != 3; }, "0 (auto), 2 or 4", nullptr},
    {"tile_order", &Ctx::use_order, nullptr, 0, 2, nullptr, "0, 1 or 2", apply_orders},
    {"stale_deg", &Ctx::stale_deg, nullptr, 0, 180, nullptr, nullptr, nullptr},
    {"quad", &Ctx::quad_pct, nullptr, 0, 100, nullptr, "a percentage", apply_orders},
    {"filter_bits", &Ctx::filter_bits, nullptr, 0, 8, [](int v) { return v == 0 || v == 8; },
     "0 (exact weights) or 8 (texture-unit weights)", apply_orders},
    {"sat_chunk", &Ctx::sat_chunk, nullptr, 1, 64, nullptr, nullptr, nullptr},
    {"sat_layout", &Ctx::sat_layout, nullptr, 0, 1, nullptr, "0 (cell4 copy) or 1 (the plain float SAT)",
     [](Ctx* c, int& value) {
       if (value == 1 && c->sat.d_cells) {   // the copy is not needed any more (17 GiB at 1024^3)
         QUIESCE(c);
         sat_drop(c, kSatCells);
       }
       return CVR_OK;
     }},
    {"sat_keep_scratch", &Ctx::sat_keep_scratch, nullptr, 0, 1, nullptr, nullptr,
     [](Ctx* c, int& value) {
       if (!value && c->sat.d_scratch) {
         QUIESCE(c);
         sat_drop(c, kSatScratch);
       }
       return CVR_OK;
     }},
    {"shade_flat", &Ctx::shade_flat, nullptr, 0, 1, nullptr, nullptr, nullptr},
    {"flat_group", &Ctx::flat_group, nullptr, 1, 4096, nullptr, "in [1, 4096]", nullptr},
    // tests: force the flat pipeline's fallback
    {"debug_flat_limit", &Ctx::debug_flat_limit, nullptr, 0, kAny, nullptr, ">= 0", nullptr},
    {"shade_counters", &Ctx::shade_counters, nullptr, kNone, kAny, nullptr, nullptr, apply_flag},
    {"tile_stats", &Ctx::tile_stats, nullptr, kNone, kAny, nullptr, nullptr, apply_flag},
    // the ring of HIP events around every frame's ray-march launch; reads its size
    {"kernel_timing", nullptr, [](const Ctx* c) { return (int)c->ev_start.size(); }, 0, 4096, nullptr,
     "0..4096 frames",
     [](Ctx* c, int& value) {
       HIP_TRY(c, hipSetDevice(c->device));
       HIP_TRY(c, hipStreamSynchronize(c->stream));
       for (hipEvent_t e : c->ev_start) (void)hipEventDestroy(e);
       for (hipEvent_t e : c->ev_stop) (void)hipEventDestroy(e);
       c->ev_start.clear();
       c->ev_stop.clear();
       c->timed_frames = 0;
       for (int i = 0; i < value; i++) {
         hipEvent_t a, b;
         HIP_TRY(c, hipEventCreate(&a));
         c->ev_start.push_back(a);
         HIP_TRY(c, hipEventCreate(&b));
         c->ev_stop.push_back(b);
       }
       return CVR_OK;
     }},
    {"macro", &Ctx::macro_shift, nullptr, 0, 6, [](int v) { return v != 1; },
     "0 (no empty-space skipping) or 2..6",
     [](Ctx* c, int&) {
       c->skip.occ_valid = 0;
       return CVR_OK;
     }},
    {"cell_skip", &Ctx::cell_skip, nullptr, 0, 4, nullptr,
     "0 (off), 1 (empty-sample flags), 2 (+ distance skip per lane), 3 (+ distance skip when every "
     "lane can) or 4 (+ distance skip, equal for the lanes that can)",
     nullptr},
    {"skip_min_pct", &Ctx::skip_min_pct, nullptr, 0, 101, nullptr, nullptr, nullptr},
    {"tile_cost", &Ctx::cost_time, nullptr, 0, 1, nullptr, "0 (longest ray) or 1 (time)", nullptr},
    {"max_waves_cu", &Ctx::max_waves_cu, nullptr, 0, 32, nullptr, nullptr, nullptr},
    {"launch_interleave", &Ctx::launch_interleave, nullptr, 0, 1, nullptr, nullptr, nullptr},
    {"gather_root_idle", &Ctx::gather_root_idle, nullptr, 0, 1, nullptr, nullptr, nullptr},
    // exchange g waits for exchange g + D - B, which the 64-event ring still holds
    // while B - D < 64 (cvr_comm.cpp): any B <= 64 with D >= 1 render streams
    {"gather_sets", &Ctx::gather_sets, nullptr, 0, CVR_MAX_GATHER_SETS, nullptr, nullptr, nullptr},
    {"exchange_code", &Ctx::exchange_code, nullptr, 0, 1, nullptr, nullptr, nullptr},
    // tolerance mode: NOT bit-exact with the oracle (DESIGN §5‴)
    {"native_exp", &Ctx::native_exp, nullptr, 0, 1, nullptr, nullptr, nullptr},
    {"encode_onepass", &Ctx::encode_onepass, nullptr, 0, 1, nullptr, nullptr, nullptr},
    // -1: auto
    {"exchange_lag", &Ctx::exchange_lag, nullptr, -1, CVR_MAX_GATHER_SETS - 1, nullptr, nullptr, nullptr},
    {"split_streams", &Ctx::split_streams, nullptr, 1, 32, nullptr, nullptr, nullptr},
    {"async_order", &Ctx::async_order, nullptr, 0, 1, nullptr, nullptr,
     [](Ctx* c, int&) {
       if (c->side) HIP_TRY(c, hipStreamSynchronize(c->side));
       for (auto& o : c->oslot) { o.valid = 0; o.pending = false; }
       return CVR_OK;
     }},
    {"order_interval", &Ctx::order_interval, nullptr, 1, 1000000, nullptr, ">= 1", nullptr},
    // diagnostics: truncated order builds
    {"debug_epi_stop", &Ctx::epi_stop, nullptr, kNone, kAny, nullptr, nullptr, nullptr},
    // tests: the skip flags' scratch "fails"
    {"debug_cell_flags_oom", &Ctx::debug_flags_oom, nullptr, 0, 1, nullptr, nullptr, nullptr},
    // diagnostics only: the image is incomplete
    {"debug_keep", &Ctx::debug_keep, nullptr, 0, kAny, nullptr, ">= 0", nullptr},
    {"boost", &Ctx::boost_pct, nullptr, 0, 100, nullptr, "a percentage", nullptr},
    {"band_cap", &Ctx::band_cap_pct, nullptr, 100, 200, nullptr, nullptr,
     [](Ctx* c, int& value) {
       if (value != c->band_cap_pct) invalidate_orders(c);   // the learned orders are laid out for the old cap
       return CVR_OK;
     }},
    // slices one launch of the slice-based renderer advances (sbtm.hip's blocked form; 1: plain)
    {"sbtm_slices_per_launch", &Ctx::sbtm_slices_per_launch, nullptr, 1, kSbtmMaxBatch, nullptr, nullptr, nullptr},
    // read-only
    {"cell_flags_active", nullptr, [](const Ctx* c) { return (int)(c->skip.flags_valid && !c->skip.flags_oom); },
     1, 0, nullptr, nullptr, nullptr},
    {"cell_flags_valid", nullptr, [](const Ctx* c) { return c->skip.flags_valid; }, 1, 0, nullptr, nullptr, nullptr},
    {"sat_build_us", nullptr, [](const Ctx* c) { return c->sat.build_us; }, 1, 0, nullptr, nullptr, nullptr},
    // empty macro cells (after a render)
    {"occ_empty_permille", nullptr,
     [](const Ctx* c) { return c->skip.occ_valid ? (int)(c->skip.occ_empty * 1000.0f + 0.5f) : -1; },
     1, 0, nullptr, nullptr, nullptr},
    // the context stream's job-list capacity
    {"flat_cap_kjobs", nullptr,
     [](const Ctx* c) {
       for (const auto& J : c->flat)
         if (J.owned && J.stream == c->stream) return (int)(J.cap / 1000);
       return 0;
     },
     1, 0, nullptr, nullptr, nullptr},
    {"light_cache_builds", nullptr, [](const Ctx* c) { return c->lc.builds; }, 1, 0, nullptr, nullptr, nullptr},
    {"vct_pyramid_builds", nullptr, [](const Ctx* c) { return c->vct.builds; }, 1, 0, nullptr, nullptr, nullptr},
    // the last slice-based frame: slices drawn, and the launches that drew them
    {"sbtm_slices", nullptr, [](const Ctx* c) { return c->sbtm.slices; }, 1, 0, nullptr, nullptr, nullptr},
    {"sbtm_launches", nullptr, [](const Ctx* c) { return c->sbtm.launches; }, 1, 0, nullptr, nullptr, nullptr},
    // the packed template arguments of the last rc1pass_tile_kernel launched (-1: none yet)
    {"rc1pass_variant", nullptr, [](const Ctx* c) { return c->rc1pass_variant; }, 1, 0, nullptr, nullptr, nullptr},
    // the kept G-buffer's pixels with a hit (waits for its geometry pass; -1: none kept), and
    // the geometry launches so far
    {"deferred_hits", nullptr,
     [](const Ctx* c) {
       unsigned long long n = 0;
       if (!c->deferred.valid || hipSetDevice(c->device) != hipSuccess ||
           hipStreamSynchronize(c->stream) != hipSuccess ||
           hipMemcpy(&n, c->deferred.d_hits, sizeof(n), hipMemcpyDeviceToHost) != hipSuccess)
         return -1;
       return (int)n;
     },
     1, 0, nullptr, nullptr, nullptr},
    {"deferred_launches", nullptr, [](const Ctx* c) { return c->deferred.launches; }, 1, 0, nullptr, nullptr, nullptr},
    // the curvature launches so far, and the pixels of the last advanced lighting pass whose
    // feature colour has red or green set (waits for that pass; -1: none yet)
    {"advdeferred_curvature_launches", nullptr, [](const Ctx* c) { return c->adv.launches; }, 1, 0, nullptr, nullptr,
     nullptr},
    {"advdeferred_ridge_pixels", nullptr,
     [](const Ctx* c) {
       unsigned long long n = 0;
       if (!c->adv.shaded || hipSetDevice(c->device) != hipSuccess ||
           hipStreamSynchronize(c->stream) != hipSuccess ||
           hipMemcpy(&n, c->adv.d_features, sizeof(n), hipMemcpyDeviceToHost) != hipSuccess)
         return -1;
       return (int)n;
     },
     1, 0, nullptr, nullptr, nullptr},
};

const Option* find_option(const char* key) {
  for (const Option& o : kOptions)
    if (!std::strcmp(key, o.key)) return &o;
  return nullptr;
}

// "<key> must be 0 or 1" / "<key> must be <lo>..<hi>" for the rows without a text
cvr_status refuse(Ctx* c, const Option& o) {
  if (o.expect) return fail(c, CVR_ERR_ARG, "%s must be %s", o.key, o.expect);
  if (o.lo == 0 && o.hi == 1) return fail(c, CVR_ERR_ARG, "%s must be 0 or 1", o.key);
  return fail(c, CVR_ERR_ARG, "%s must be %d..%d", o.key, o.lo, o.hi);
}

}  // namespace

extern "C" {
#pragma GCC visibility push(default)

cvr_status cvr_set_option(cvr_ctx* ctx, const char* key, int value) {
  Ctx* c = reinterpret_cast<Ctx*>(ctx);
  if (!c || !key) return CVR_ERR_ARG;
  if (c->group) {
    for (const char* k : {"split_streams", "gather_sets", "gather_root_idle", "exchange_lag"})
      if (!std::strcmp(key, k))
        return fail(c, CVR_ERR_ARG, "option '%s' belongs to the group's own exchange", key);
    return cvr::group_each(c, [&](cvr_ctx* _m) { return cvr_set_option(_m, key, value); });
  }
  const Option* o = find_option(key);
  if (!o || o->lo > o->hi) return fail(c, CVR_ERR_ARG, "unknown option '%s'", key);
  if (value < o->lo || value > o->hi || (o->ok && !o->ok(value))) return refuse(c, *o);
  if (o->apply) {
    const cvr_status st = o->apply(c, value);
    if (st != CVR_OK) return st;
  }
  if (o->field) c->*(o->field) = value;
  return CVR_OK;
}

int cvr_get_option(const cvr_ctx* ctx, const char* key) {
  const Ctx* c = reinterpret_cast<const Ctx*>(ctx);
  if (!c || !key) return -1;
  if (c->group) return cvr_get_option(cvr_group_member(const_cast<cvr_ctx*>(ctx), 0), key);
  const Option* o = find_option(key);
  if (!o) return -1;
  return o->field ? c->*(o->field) : o->get(c);
}

#pragma GCC visibility pop
}  // extern "C"
