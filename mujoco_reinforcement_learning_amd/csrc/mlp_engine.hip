// The ppo_ctx C-ABI of the MLP actor-critic engine: the context's lifecycle and workspace
// (ppo_ctx_create / ppo_ctx_destroy, parameter layout and binding), argument validation, and the
// dispatch of every entry point to the path that runs it:
//   fused    bf16, two equal hidden layers of a compiled width  fused_policy.h, fused_update.h
//   wide     bf16, ReLU nets the fused kernels do not cover      wide_path.h
//   layered  everything else, and all of f32                     layered_path.h
// The host glue of the fused path lives here too: FusedArgs / AdamPackArgs assembly, the staged
// records and the gathered-copy record, the step tail and the persistent rollout entry points.
// No kernel is defined in this file.
#include <algorithm>
#include <new>

#include "common.h"
#include "ctx.h"
#include "fused_policy.h"
#include "fused_update.h"
#include "layered_path.h"
#include "ppo_loss.h"
#include "reduce_slabs.h"
#include "timing.h"
#include "wide_path.h"

namespace ppo {

static const int g_fused_enabled = env_knob("PPO_FUSED", 1);
// PPO_FUSED_DIRECT=0: the 8-wave fused update reads the gathered xb / srow copies (written by the
// prep kernel or the previous step tail) instead of the staged records through the row indices
// (the ctx default; ppo_ctx_fused_direct switches it)
static const int g_fused_direct = env_knob("PPO_FUSED_DIRECT", 1);

// Pointers of both nets for the fused kernels (bf16 images from ctx->fw, f32 masters in params).
static void fused_nets(const ppo_ctx *ctx, FusedNet (&out)[2]) {
  for (int z = 0; z < 2; ++z) {
    const NetDesc &nd = ctx->net[z];
    FusedNet &fn = out[z];
    fn.fconst = ctx->fconst[z];
    fn.w0b = ctx->fw[z][0];
    fn.w1b = ctx->fw[z][1];
    fn.w1bt = ctx->fw[z][2];
    fn.w0 = ctx->params + nd.layer[0].w_off;
    fn.w1 = ctx->params + nd.layer[1].w_off;
    fn.b0 = nd.layer[0].b_off >= 0 ? ctx->params + nd.layer[0].b_off : nullptr;
    fn.b1 = nd.layer[1].b_off >= 0 ? ctx->params + nd.layer[1].b_off : nullptr;
    fn.wh = ctx->params + nd.layer[2].w_off;
    fn.bh = nd.layer[2].b_off >= 0 ? ctx->params + nd.layer[2].b_off : nullptr;
    fn.off_w0 = nd.layer[0].w_off;
    fn.off_b0 = nd.layer[0].b_off;
    fn.off_w1 = nd.layer[1].w_off;
    fn.off_b1 = nd.layer[1].b_off;
    fn.off_wh = nd.layer[2].w_off;
    fn.off_bh = nd.layer[2].b_off;
  }
}

// Where each parameter of both nets lands in the packed constants images (fused_update.h).
static void fused_const_maps(const ppo_ctx *ctx, ConstImgMap (&out)[2]) {
  for (int z = 0; z < 2; ++z) {
    const NetDesc &nd = ctx->net[z];
    ConstImgMap &m = out[z];
    m.img = ctx->fconst[z];
    m.begin = nd.begin;
    m.end = nd.begin + nd.count;
    m.off_w0 = nd.layer[0].w_off;
    m.off_b0 = nd.layer[0].b_off;
    m.off_w1 = nd.layer[1].w_off;
    m.off_b1 = nd.layer[1].b_off;
    m.off_wh = nd.layer[2].w_off;
    m.off_bh = nd.layer[2].b_off;
    m.off_logstd = z == 0 ? nd.logstd_off : -1;
    m.nh = z == 0 ? ctx->cfg.act_dim : 1;
    m.din = ctx->cfg.obs_dim * ctx->cfg.window;
    m.w0b = ctx->fw[z][0];
  }
}

static bool fused_active(const ppo_ctx *ctx) {
  return ctx->prec == PPO_PREC_BF16 && ctx->fused_ok && g_fused_enabled;
}

// Precision bf16 with supported shapes: gather + bf16 weight refresh, the persistent fused
// forward/loss/backward kernel (one partial-gradient slab per workgroup), then the fixed-order
// slab reduction.  Same contract as the layered path (layered_path.h).
static FusedArgs fused_args(ppo_ctx *ctx, const float *states_d, const float *actions_d,
                            const float *old_logp_d, const float *adv_d, const float *vtarget_d,
                            const int32_t *rows_d, int b, const int32_t *count_d,
                            const LossCoef &coef, bool staged, bool pack_w) {
  FusedArgs q{};
  fused_nets(ctx, q.net);
  q.logstd = ctx->params + ctx->net[0].logstd_off;
  q.off_logstd = ctx->net[0].logstd_off;
  q.xb = ctx->fxb;
  q.srow = ctx->fsrow;
  q.states = states_d;
  q.actions = actions_d;
  q.old_logp = old_logp_d;
  q.adv = adv_d;
  q.vtarget = vtarget_d;
  q.rows = rows_d;
  q.rows_n = count_d;
  q.rec = staged ? ctx->frec : nullptr;
  q.n_rec = staged ? ctx->frec_rows : 0;
  q.pack_w = pack_w;
  q.params = ctx->params;
  fused_const_maps(ctx, q.cmap);
  q.b = b;
  q.din = ctx->cfg.obs_dim * ctx->cfg.window;
  q.act_dim = ctx->cfg.act_dim;
  q.act = ctx->cfg.activation;
  q.hidden = ctx->fused_hidden;
  q.omv = ctx->cfg.output_max_value;
  q.coef = coef;
  q.slabs = ctx->fslabs;
  q.slab_stride = ctx->total_params;
  q.loss_part = ctx->floss;
  q.stamps = ctx->fstamp_on ? ctx->fstamps : nullptr;
  q.G = std::min(kFusedMaxWG, ceil_div(b, kFusedRows));
  q.direct = staged && ctx->fdirect;
  return q;
}

// gather (q.b rows; 0 = none) and, with q.pack_w, the weight-image refresh
static int fused_prep(const ppo_ctx *ctx, const FusedArgs &q, hipStream_t st) {
  const double H = ctx->fused_hidden;
  const int din = q.din, A = q.act_dim;
  // algorithmic traffic: gather (row index, din + A + 3 floats -- or one 128 B record -- in;
  // 64 + 64 B out per row) and weight images (f32 in, 3 bf16 images out per net)
  const double wbytes =
      q.pack_w ? 2.0 * (4.0 * H * (din + H) + 2.0 * H * (kFusedKX + 2.0 * H)) : 0.0;
  const double in_row = q.rec ? 4.0 + kRecordBytes : 4.0 * (1 + din + A + 3);
  const TimRec rec{KC_GATHER, "fused_prep_kernel", 0.0,
                   static_cast<double>(q.b) * (in_row + 2.0 * kFusedKX + 4.0 * kFusedSP) + wbytes};
  return fused_prep_launch(q, rec, st);
}

// The gathered-copy record (ctx.h fg_rows): a caller's PPO_STAGED_ROWS_GATHERED is a promise
// about stream order that nothing on the device checks, so the host keeps which rows the last
// staged gather wrote and gathers again when the promise names other rows.  The check is POINTER
// identity (the index buffer's address and count), not content: a caller that rewrites the same
// index buffer in place (e.g. a fresh permutation into one buffer) must not pass
// PPO_STAGED_ROWS_GATHERED for it.  A gather is recorded only once its launch was issued
// successfully; a failed entry point clears the record.
static bool gathered_holds(const ppo_ctx *ctx, const int32_t *rows_d, int b) {
  return rows_d != nullptr && ctx->fg_rows == rows_d && ctx->fg_b == b;
}
static void note_gathered(ppo_ctx *ctx, const int32_t *rows_d, int b) {
  ctx->fg_rows = rows_d;
  ctx->fg_b = rows_d ? b : 0;
}

static int fused_forward_backward(ppo_ctx *ctx, const FusedArgs &q, hipStream_t st) {
  const int H = ctx->fused_hidden, din = q.din, A = q.act_dim, b = q.b;
  const int64_t P = ctx->total_params;
  ctx->fstamp_g = q.G;
  // FLOPs per row per net: forward (din*H + H*H + a*H), dgrad (H*H + a*H), wgrad (din*H +
  // H*H + a*H), a = A (actor) / 1 (critic); bytes: staged rows + one slab per workgroup
  double fl = 0.0;
  for (int z = 0; z < 2; ++z) {
    const double a = z == 0 ? A : 1;
    fl += 2.0 * b * ((din * H + H * H + a * H) + (H * H + a * H) + (din * H + H * H + a * H));
  }
  // HBM bytes: the staged rows once, the bf16 weight images once (every workgroup re-reads
  // them from L2, which is not HBM traffic) and one partial-gradient slab per workgroup
  const double by = static_cast<double>(b) * (2.0 * kFusedKX + 4.0 * kFusedSP) +
                    4.0 * q.G * static_cast<double>(P) + 2.0 * 2.0 * H * (kFusedKX + 2.0 * H);
  const int na = A <= 2 ? 2 : A <= 4 ? 4 : A <= 6 ? 6 : 8;
  const TimRec rec{KC_FUSED,
                   tim_active() ? intern_name("fused_update_kernel<%d, %d, %d, false, %d>", H, q.act, na,
                                              fused_sched(q.act))
                                : nullptr,
                   fl, by};
  return fused_update_launch(q, rec, st);
}

static int fused_reduce_args(const ppo_ctx *ctx, const FusedArgs &q, float *grad_d, float *loss_d,
                            ReduceArgs &r) {
  const int A = q.act_dim;
  const int64_t P = ctx->total_params;
  r = ReduceArgs{};
  for (int z = 0; z < 2; ++z) {
    const NetDesc &nd = ctx->net[z];
    auto seg = [&](int64_t off, int64_t len) {
      return add_seg(r, off, len, ctx->fslabs + off, P, q.G);
    };
    if (z == 0)
      if (int rc = seg(nd.logstd_off, A)) return rc;
    for (int l = 0; l <= nd.n_hidden; ++l) {
      const LayerDesc &L = nd.layer[l];
      if (int rc = seg(L.w_off, static_cast<int64_t>(L.out) * L.in)) return rc;
      if (L.b_off >= 0)
        if (int rc = seg(L.b_off, L.out)) return rc;
    }
  }
  set_loss_tail(r, P, grad_d, ctx->floss, q.G, q.coef, ctx->params + ctx->net[0].logstd_off, A,
                ctx->ent_log_share, loss_d);
  return 0;
}

static int fused_minibatch_grad(ppo_ctx *ctx, const float *states_d, const float *actions_d,
                                const float *old_logp_d, const float *adv_d,
                                const float *vtarget_d, const int32_t *rows_d, int b,
                                const int32_t *count_d, const LossCoef &coef, float *grad_d,
                                float *loss_d, hipStream_t st, bool staged = false,
                                bool pack_w = true, bool gathered = false) {
  const FusedArgs q = fused_args(ctx, states_d, actions_d, old_logp_d, adv_d, vtarget_d, rows_d,
                                 b, count_d, coef, staged, pack_w);
  gathered = gathered && staged && gathered_holds(ctx, rows_d, b);
  if ((!gathered && !q.direct) || pack_w) {
    FusedArgs p = q;
    p.b = (gathered || q.direct) ? 0 : b;
    if (int rc = fused_prep(ctx, p, st)) return rc;
    if (p.b > 0) note_gathered(ctx, staged && count_d == nullptr ? rows_d : nullptr, b);
  }
  ReduceArgs r;
  if (int rc = fused_reduce_args(ctx, q, grad_d, loss_d, r)) return rc;
  if (int rc = fused_forward_backward(ctx, q, st)) return rc;
  const int64_t P = ctx->total_params;
  return reduce_slabs_launch(r, TimRec{KC_REDUCE, "reduce_slabs_kernel", static_cast<double>(q.G) * P,
                                       4.0 * (static_cast<double>(q.G) + 1) * P}, st);
}

// AdamPackArgs for the ctx's bound parameters (both nets) and the fused weight images
static AdamPackArgs adam_pack_args(const ppo_ctx *ctx, const float *g_d, float *m_d, float *v_d,
                                   const float *sched_d, float neg_a, float neg_c, float bc2,
                                   float omb1, float b2, float omb2, float eps) {
  AdamPackArgs a{};
  a.p = ctx->params;
  a.g = g_d;
  a.m = m_d;
  a.v = v_d;
  a.n = ctx->total_params;
  a.n_actor = ctx->net[0].count;
  a.sched = sched_d;
  a.neg_a = neg_a;
  a.neg_c = neg_c;
  a.bc2 = bc2;
  a.w1 = omb1;
  a.b2 = b2;
  a.omb2 = omb2;
  a.eps = eps;
  FusedNet nets[2];
  fused_nets(ctx, nets);
  for (int z = 0; z < 2; ++z) {
    a.w1b[z] = const_cast<__bf16 *>(nets[z].w1b);
    a.w1bt[z] = const_cast<__bf16 *>(nets[z].w1bt);
    a.off_w1[z] = nets[z].off_w1;
  }
  fused_const_maps(ctx, a.cmap);
  a.din = ctx->cfg.obs_dim * ctx->cfg.window;
  a.H = ctx->fused_hidden;
  return a;
}

static int check_ctx(const ppo_ctx *ctx) {
  PPO_REQUIRE(ctx != nullptr, "null ppo_ctx");
  PPO_REQUIRE(ctx->params != nullptr, "ppo_ctx: parameters not bound (ppo_bind_params)");
  return 0;
}

}  // namespace ppo

using namespace ppo;

extern "C" int ppo_ctx_create(const ppo_net_cfg *cfg, int device, ppo_ctx **out) {
  PPO_REQUIRE(cfg && out, "ppo_ctx_create: null argument");
  PPO_REQUIRE(cfg->obs_dim > 0 && cfg->window > 0, "ppo_ctx_create: bad obs/window");
  PPO_REQUIRE(cfg->act_dim > 0 && cfg->act_dim <= kMaxAct, "ppo_ctx_create: act_dim must be in [1, %d]",
              kMaxAct);
  PPO_REQUIRE(cfg->n_actor_hidden >= 1 && cfg->n_actor_hidden <= PPO_MAX_LAYERS &&
                  cfg->n_critic_hidden >= 1 && cfg->n_critic_hidden <= PPO_MAX_LAYERS,
              "ppo_ctx_create: hidden layer count must be in [1, %d]", PPO_MAX_LAYERS);
  PPO_REQUIRE(cfg->activation >= PPO_ACT_RELU && cfg->activation <= PPO_ACT_ELU,
              "ppo_ctx_create: unknown activation %d", cfg->activation);
  PPO_REQUIRE(cfg->max_rows > 0, "ppo_ctx_create: max_rows must be positive");
  PPO_HIP_TRY(hipSetDevice(device));
  ppo_ctx *ctx = new (std::nothrow) ppo_ctx();
  PPO_REQUIRE(ctx != nullptr, "ppo_ctx_create: out of host memory");
  ctx->cfg = *cfg;
  ctx->device = device;
  ctx->ent_log_share = 1.f;
  const int din = cfg->obs_dim * cfg->window;
  ParamLayout lay;
  const int64_t R = cfg->max_rows;
  // layered arena: 256 spare bytes at the end
  Workspace ws(kWsAlign, 0, 256);
  for (int z = 0; z < 2; ++z) {
    NetDesc &nd = ctx->net[z];
    nd.begin = lay.total();
    const int nh = z == 0 ? cfg->n_actor_hidden : cfg->n_critic_hidden;
    const int32_t *hid = z == 0 ? cfg->actor_hidden : cfg->critic_hidden;
    const bool bias = z == 0 ? cfg->actor_use_bias != 0 : true;
    nd.n_hidden = nh;
    nd.logstd_off = z == 0 ? lay.add(cfg->act_dim) : -1;
    int width = din;
    for (int l = 0; l <= nh; ++l) {
      const int o = (l < nh) ? hid[l] : (z == 0 ? cfg->act_dim : 1);
      if (l < nh && (o <= 0 || o > 1024)) {
        delete ctx;
        set_error("ppo_ctx_create: hidden width %d out of range [1, 1024]", o);
        return PPO_EINVAL;
      }
      LayerDesc &L = nd.layer[l];
      L.in = width;
      L.out = o;
      L.w_off = lay.add(static_cast<int64_t>(o) * width);
      L.b_off = bias ? lay.add(o) : -1;
      if (l < nh) ws.take_n(&nd.h[l], R * o);  // hidden outputs (max_rows, width)
      width = o;
    }
    ws.take_n(&nd.g, R * nd.layer[nh].in);    // g = dH_L (last hidden width)
    ws.take_n(&nd.dz, R * nd.layer[nh].out);  // dz
    nd.count = lay.total() - nd.begin;
  }
  const int64_t off = lay.total();
  ctx->total_params = off;
  {
    const int A = cfg->act_dim;
    const int da = ctx->net[0].layer[ctx->net[0].n_hidden].in;
    const int dc = ctx->net[1].layer[ctx->net[1].n_hidden].in;
    ctx->hw_off_ba = static_cast<int>(align_up(static_cast<int64_t>(A) * da, 4));
    ctx->hw_off_wc = ctx->hw_off_ba + static_cast<int>(align_up(A, 4));
    ctx->hw_off_bc = ctx->hw_off_wc + static_cast<int>(align_up(dc, 4));
    ctx->hw_stride = ctx->hw_off_bc + 4;
  }
  ctx->ldx = static_cast<int>(align_up(din, 4));
  ws.take_n(&ctx->slabs, static_cast<int64_t>(kSlabSplits) * off);
  ws.take_n(&ctx->head_part, static_cast<int64_t>(kHeadSplits) * (cfg->act_dim + 2));
  ws.take_n(&ctx->head_w_part, static_cast<int64_t>(kHeadSplits) * ctx->hw_stride);
  ws.take_n(&ctx->xg, R * ctx->ldx);  // gathered minibatch states (max_rows, ldx)
  if (int rc = workspace_alloc(ws, "ppo_ctx_create", -1, false, &ctx->arena)) {
    ppo_ctx_destroy(ctx);
    return rc;
  }
  // fused bf16 update: both nets 2 hidden layers of one compiled width, W*O <= 32, A <= 8
  const NetDesc &na = ctx->net[0], &nc = ctx->net[1];
  const int H = na.layer[0].out;
  ctx->fused_ok = na.n_hidden == 2 && nc.n_hidden == 2 && fused_width_ok(H) &&
                  na.layer[1].out == H && nc.layer[0].out == H && nc.layer[1].out == H &&
                  din <= kFusedKX && cfg->act_dim <= kFusedMaxAct;
  ctx->fused_hidden = H;
  if (ctx->fused_ok) {
    // fused arena: W images rounded to 128 elements, 1 KB at the end
    Workspace fws(kWsAlign, 0, 1024);
    for (int z = 0; z < 2; ++z)  // per net one block: W0 image (H, 32), W1 (H, H), W1^T (H, H)
      fws.take_n(&ctx->fw[z][0], align_up(static_cast<int64_t>(H) * (kFusedKX + 2 * H), 128));
    for (int z = 0; z < 2; ++z) fws.take(&ctx->fconst[z], fused_const_bytes(H));
    fws.take_n(&ctx->fxb, R * kFusedKX);    // (max_rows, 32) staged bf16 states
    fws.take_n(&ctx->fsrow, R * kFusedSP);  // (max_rows, 16) staged row scalars
    fws.take_n(&ctx->fslabs, static_cast<int64_t>(kFusedMaxWG) * off);
    fws.take_n(&ctx->floss, kFusedMaxWG * 2);
    if (int rc = workspace_alloc(fws, "ppo_ctx_create (fused workspace)", -1, false,
                                 &ctx->farena)) {
      ppo_ctx_destroy(ctx);
      return rc;
    }
    for (int z = 0; z < 2; ++z) {
      ctx->fw[z][1] = ctx->fw[z][0] + static_cast<int64_t>(H) * kFusedKX;
      ctx->fw[z][2] = ctx->fw[z][0] + static_cast<int64_t>(H) * (kFusedKX + H);
    }
    // the constants images, their pads written here once (the writers store parameters only)
    char *pads = new (std::nothrow) char[fused_const_bytes(H)];
    hipError_t e = pads ? hipSuccess : hipErrorOutOfMemory;
    for (int z = 0; z < 2 && e == hipSuccess; ++z) {
      fused_const_pads(H, pads);
      e = hipMemcpy(ctx->fconst[z], pads, fused_const_bytes(H), hipMemcpyHostToDevice);
    }
    delete[] pads;
    if (e != hipSuccess) {
      ppo_ctx_destroy(ctx);
      set_error("ppo_ctx_create: writing the fused constants images failed: %s",
                hipGetErrorString(e));
      return PPO_EHIP;
    }
    ctx->fdirect = g_fused_direct != 0;
  }
  *out = ctx;
  return 0;
}

extern "C" int ppo_ctx_destroy(ppo_ctx *ctx) {
  if (!ctx) return 0;
  (void)hipSetDevice(ctx->device);
  if (g_free_tim == &ctx->tim) g_free_tim = nullptr;
  timing_release(ctx->tim);
  if (ctx->arena) (void)hipFree(ctx->arena);
  if (ctx->farena) (void)hipFree(ctx->farena);
  if (ctx->fstamps) (void)hipFree(ctx->fstamps);
  if (ctx->frec) (void)hipFree(ctx->frec);
  wide_free(ctx);
  delete ctx;
  return 0;
}

extern "C" int64_t ppo_param_count(const ppo_ctx *ctx, int net) {
  if (!ctx) return -1;
  if (net == 0 || net == 1) return ctx->net[net].count;
  return ctx->total_params;
}

extern "C" int ppo_param_offsets(const ppo_ctx *ctx, int64_t *offsets, int max_tensors) {
  PPO_REQUIRE(ctx != nullptr, "ppo_param_offsets: null ctx");
  int n = 0;
  auto put = [&](int64_t off) {
    if (offsets && n < max_tensors) offsets[n] = off;
    ++n;
  };
  for (int z = 0; z < 2; ++z) {
    const NetDesc &nd = ctx->net[z];
    if (z == 0) put(nd.logstd_off);
    for (int l = 0; l <= nd.n_hidden; ++l) {
      put(nd.layer[l].w_off);
      if (nd.layer[l].b_off >= 0) put(nd.layer[l].b_off);
    }
  }
  return n;
}

extern "C" int ppo_bind_params(ppo_ctx *ctx, float *params_d) {
  PPO_REQUIRE(ctx && params_d, "ppo_bind_params: null argument");
  ctx->params = params_d;
  return 0;
}

extern "C" int ppo_policy_step(ppo_ctx *ctx, const float *state_d, int n, const float *eps_d,
                               uint64_t seed, uint64_t offset, float *action_d, float *logp_d,
                               float *value_d, float *mean_d, void *stream) {
  if (int rc = check_ctx(ctx)) return rc;
  PPO_REQUIRE(state_d && n > 0, "ppo_policy_step: bad state / n");
  PPO_REQUIRE(n <= ctx->cfg.max_rows, "ppo_policy_step: n=%d exceeds max_rows=%d", n,
              ctx->cfg.max_rows);
  hipStream_t st = as_stream(stream);
  TimingScope timing_scope(ctx->tim);
  if (wide_active(ctx))
    return wide_policy_step(ctx, state_d, n, eps_d, seed, offset, action_d, logp_d, value_d,
                            mean_d, true, st);
  return layered_policy_step(ctx, state_d, n, eps_d, seed, offset, action_d, logp_d, value_d,
                             mean_d, st);
}

extern "C" int ppo_pack_weights(ppo_ctx *ctx, void *stream) {
  if (int rc = check_ctx(ctx)) return rc;
  if (wide_active(ctx)) {
    TimingScope timing_scope(ctx->tim);
    return wide_pack(ctx, as_stream(stream));
  }
  if (!fused_active(ctx)) return 0;  // the layered path reads the f32 masters directly
  TimingScope timing_scope(ctx->tim);
  FusedArgs q{};
  fused_nets(ctx, q.net);
  q.b = 0;
  q.pack_w = true;
  q.params = ctx->params;
  fused_const_maps(ctx, q.cmap);
  q.din = ctx->cfg.obs_dim * ctx->cfg.window;
  q.hidden = ctx->fused_hidden;
  const double H = ctx->fused_hidden;
  const TimRec rec{KC_GATHER, "fused_prep_kernel", 0.0,
                   2.0 * (4.0 * H * (q.din + H) + 2.0 * H * (kFusedKX + 2.0 * H))};
  return fused_prep_launch(q, rec, as_stream(stream));
}

extern "C" int ppo_ctx_fused_active(const ppo_ctx *ctx) {
  return (ctx && fused_active(ctx)) ? 1 : 0;
}

// The ctx's record buffer grown to n_rows (outside a graph capture: the first call per size).
static int ensure_records(ppo_ctx *ctx, int64_t n_rows, hipStream_t st, const char *who) {
  if (n_rows > ctx->frec_cap) {
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    PPO_REQUIRE(hipStreamIsCapturing(st, &cap) == hipSuccess &&
                    cap == hipStreamCaptureStatusNone,
                "%s: first call for %lld rows inside a graph capture", who,
                static_cast<long long>(n_rows));
    (void)hipStreamSynchronize(st);
    if (ctx->frec) (void)hipFree(ctx->frec);
    ctx->frec = nullptr;
    ctx->frec_cap = 0;
    void *p = nullptr;
    const hipError_t e = hipMalloc(&p, static_cast<size_t>(n_rows) * kRecordBytes);
    PPO_REQUIRE(e == hipSuccess, "%s: hipMalloc(%lld records): %s", who,
                static_cast<long long>(n_rows), hipGetErrorString(e));
    ctx->frec = static_cast<uint4 *>(p);
    ctx->frec_cap = n_rows;
  }
  ctx->frec_rows = n_rows;
  return 0;
}

extern "C" int ppo_stage_records(ppo_ctx *ctx, const float *states_d, const float *actions_d,
                                 const float *old_logp_d, const float *adv_d,
                                 const float *vtarget_d, int64_t n_rows, void *stream) {
  if (int rc = check_ctx(ctx)) return rc;
  PPO_REQUIRE(fused_active(ctx), "ppo_stage_records: needs the fused bf16 path "
                                 "(ppo_ctx_fused_active)");
  note_gathered(ctx, nullptr, 0);  // new records: any gathered copy is stale
  PPO_REQUIRE(states_d && actions_d && old_logp_d && adv_d && vtarget_d && n_rows > 0,
              "ppo_stage_records: null buffer or n_rows <= 0");
  hipStream_t st = as_stream(stream);
  if (int rc = ensure_records(ctx, n_rows, st, "ppo_stage_records")) return rc;
  TimingScope timing_scope(ctx->tim);
  const int din = ctx->cfg.obs_dim * ctx->cfg.window, A = ctx->cfg.act_dim;
  const TimRec rec{KC_GATHER, "fused_records_kernel", 0.0,
                   static_cast<double>(n_rows) * (4.0 * (din + A + 3) + kRecordBytes)};
  return fused_records_launch(ctx->frec, states_d, actions_d, old_logp_d, adv_d, vtarget_d,
                              n_rows, din, A, rec, st);
}

extern "C" int ppo_gae_stage_records(ppo_ctx *ctx, const float *value_d,
                                     const float *next_value_d, const void *reward_d,
                                     int reward_is_f64, const uint8_t *done_d,
                                     const uint8_t *terminated_d, int force_last_done, int n,
                                     int t, double gamma, double lmbda, float *adv_d,
                                     float *vtarget_d, const float *states_d,
                                     const float *actions_d, const float *old_logp_d,
                                     void *stream) {
  if (int rc = check_ctx(ctx)) return rc;
  PPO_REQUIRE(fused_active(ctx), "ppo_gae_stage_records: needs the fused bf16 path "
                                 "(ppo_ctx_fused_active)");
  note_gathered(ctx, nullptr, 0);  // new records: any gathered copy is stale
  PPO_REQUIRE(value_d && next_value_d && reward_d && terminated_d && adv_d && vtarget_d &&
                  states_d && actions_d && old_logp_d,
              "ppo_gae_stage_records: null buffer");
  PPO_REQUIRE(n > 0 && t > 0, "ppo_gae_stage_records: bad shape n=%d t=%d", n, t);
  const int64_t n_rows = static_cast<int64_t>(n) * t;
  if (t > 16 * 16) {  // beyond the pipelined scan: the two passes
    if (int rc = ppo_gae(value_d, next_value_d, reward_d, reward_is_f64, done_d, terminated_d,
                         force_last_done, n, t, gamma, lmbda, adv_d, vtarget_d, stream))
      return rc;
    return ppo_stage_records(ctx, states_d, actions_d, old_logp_d, adv_d, vtarget_d, n_rows,
                             stream);
  }
  hipStream_t st = as_stream(stream);
  if (int rc = ensure_records(ctx, n_rows, st, "ppo_gae_stage_records")) return rc;
  TimingScope timing_scope(ctx->tim);
  const int din = ctx->cfg.obs_dim * ctx->cfg.window, A = ctx->cfg.act_dim;
  GaeRecordArgs g{};
  g.value = value_d;
  g.next_value = next_value_d;
  g.reward = reward_d;
  g.done = done_d;
  g.term = terminated_d;
  g.force_last = force_last_done;
  g.n = n;
  g.t_len = t;
  g.gamma_f = static_cast<float>(gamma);
  g.lg_f = static_cast<float>(lmbda * gamma);
  g.adv = adv_d;
  g.vtarget = vtarget_d;
  g.states = states_d;
  g.actions = actions_d;
  g.old_logp = old_logp_d;
  g.rec = ctx->frec;
  g.din = din;
  g.act_dim = A;
  // algorithmic bytes: the GAE's (V, V', reward, terminated [+ done] in; adv, vtarget out) plus
  // the record pass's (state, actions, old_logp in; the 128 B record out)
  const double per_row = 4 + 4 + (reward_is_f64 ? 8 : 4) + 1 + (done_d ? 1 : 0) + 4 + 4 +
                         4.0 * (din + A + 1) + kRecordBytes;
  const TimRec rec{KC_GAE, "gae_records_kernel", 0.0, static_cast<double>(n_rows) * per_row};
  return gae_records_launch(g, reward_is_f64 != 0, rec, st);
}

extern "C" int ppo_minibatch_grad_staged(ppo_ctx *ctx, const int32_t *rows_d, int b,
                                         const int32_t *count_d, float clip_lo, float clip_hi,
                                         float entropy_coef, float inv_b, float inv_ba,
                                         float *grad_d, float *loss_d, int flags, void *stream) {
  if (int rc = check_ctx(ctx)) return rc;
  PPO_REQUIRE(fused_active(ctx) && ctx->frec && ctx->frec_rows > 0,
              "ppo_minibatch_grad_staged: no staged records (ppo_stage_records first)");
  PPO_REQUIRE(rows_d && grad_d && loss_d, "ppo_minibatch_grad_staged: null buffer");
  PPO_REQUIRE(b > 0 && b <= ctx->cfg.max_rows,
              "ppo_minibatch_grad_staged: b=%d outside [1, max_rows=%d]", b, ctx->cfg.max_rows);
  PPO_REQUIRE((flags & ~(PPO_STAGED_WEIGHTS_CURRENT | PPO_STAGED_ROWS_GATHERED)) == 0,
              "ppo_minibatch_grad_staged: flags %d", flags);
  PPO_REQUIRE(!(flags & PPO_STAGED_ROWS_GATHERED) || count_d == nullptr,
              "ppo_minibatch_grad_staged: pre-gathered rows take no device count");
  TimingScope timing_scope(ctx->tim);
  return fused_minibatch_grad(ctx, nullptr, nullptr, nullptr, nullptr, nullptr, rows_d, b,
                              count_d, LossCoef{clip_lo, clip_hi, entropy_coef, inv_b, inv_ba},
                              grad_d, loss_d, as_stream(stream), true,
                              (flags & PPO_STAGED_WEIGHTS_CURRENT) == 0,
                              (flags & PPO_STAGED_ROWS_GATHERED) != 0);
}

extern "C" int ppo_adam_pack_gather(ppo_ctx *ctx, const float *g_d, float *m_d, float *v_d,
                                    const float *sched_d, float neg_step_actor,
                                    float neg_step_critic, float bc2_sqrt, float one_minus_beta1,
                                    float beta2, float one_minus_beta2, float eps,
                                    const int32_t *next_rows_d, int next_b, void *stream) {
  if (int rc = check_ctx(ctx)) return rc;
  PPO_REQUIRE(fused_active(ctx) && ctx->frec && ctx->frec_rows > 0,
              "ppo_adam_pack_gather: no staged records (ppo_stage_records first)");
  PPO_REQUIRE(g_d && m_d && v_d, "ppo_adam_pack_gather: null buffer");
  PPO_REQUIRE(next_b >= 0 && next_b <= ctx->cfg.max_rows && (next_b == 0) == (next_rows_d == nullptr),
              "ppo_adam_pack_gather: next_b=%d", next_b);
  TimingScope timing_scope(ctx->tim);
  TailArgs t{};
  t.a = adam_pack_args(ctx, g_d, m_d, v_d, sched_d, neg_step_actor, neg_step_critic, bc2_sqrt,
                       one_minus_beta1, beta2, one_minus_beta2, eps);
  t.rows = next_rows_d;
  t.rec = ctx->frec;
  t.n_rec = ctx->frec_rows;
  t.xb = ctx->fxb;
  t.srow = ctx->fsrow;
  // direct: the next fused launch reads its rows through the indices, nothing to gather
  const bool direct = next_b > 0 && fused_args(ctx, nullptr, nullptr, nullptr, nullptr, nullptr,
                                               next_rows_d, next_b, nullptr, LossCoef{}, true,
                                               false).direct;
  t.b = direct ? 0 : next_b;
  t.reduce = false;
  ReduceArgs r{};
  r.total = ctx->total_params;
  const double P = static_cast<double>(ctx->total_params), H = ctx->fused_hidden;
  const TimRec rec{KC_ADAM, "step_tail_kernel", 0.0,
                   28.0 * P + 2.0 * 2.0 * H * (t.a.din + 2.0 * H) +
                       static_cast<double>(t.b) * (4.0 + 2.0 * kRecordBytes)};
  if (int rc = step_tail_launch(r, t, rec, as_stream(stream))) {
    note_gathered(ctx, nullptr, 0);
    return rc;
  }
  if (t.b > 0) note_gathered(ctx, next_rows_d, t.b);
  return 0;
}

extern "C" int ppo_gather_staged_rows(ppo_ctx *ctx, const int32_t *rows_d, int b, void *stream) {
  if (int rc = check_ctx(ctx)) return rc;
  PPO_REQUIRE(fused_active(ctx) && ctx->frec && ctx->frec_rows > 0,
              "ppo_gather_staged_rows: no staged records (ppo_stage_records first)");
  PPO_REQUIRE(rows_d && b > 0 && b <= ctx->cfg.max_rows,
              "ppo_gather_staged_rows: b=%d outside [1, max_rows=%d]", b, ctx->cfg.max_rows);
  TimingScope timing_scope(ctx->tim);
  const FusedArgs q = fused_args(ctx, nullptr, nullptr, nullptr, nullptr, nullptr, rows_d, b,
                                 nullptr, LossCoef{}, true, false);
  if (int rc = fused_prep(ctx, q, as_stream(stream))) return rc;
  note_gathered(ctx, rows_d, b);
  return 0;
}

extern "C" int ppo_adam_pack(ppo_ctx *ctx, const float *g_d, float *m_d, float *v_d,
                             const float *sched_d, float neg_step_actor, float neg_step_critic,
                             float bc2_sqrt, float one_minus_beta1, float beta2,
                             float one_minus_beta2, float eps, void *stream) {
  if (int rc = check_ctx(ctx)) return rc;
  PPO_REQUIRE(fused_active(ctx), "ppo_adam_pack: needs the fused bf16 path");
  PPO_REQUIRE(g_d && m_d && v_d, "ppo_adam_pack: null buffer");
  TimingScope timing_scope(ctx->tim);
  const AdamPackArgs a = adam_pack_args(ctx, g_d, m_d, v_d, sched_d, neg_step_actor,
                                        neg_step_critic, bc2_sqrt, one_minus_beta1, beta2,
                                        one_minus_beta2, eps);
  const double Hd = a.H;
  const TimRec rec{KC_ADAM, "adam_pack_kernel", 0.0,
                   28.0 * a.n + 2.0 * 2.0 * Hd * (a.din + 2.0 * Hd)};
  return adam_pack_launch(a, rec, as_stream(stream));
}

extern "C" int ppo_update_step_staged(ppo_ctx *ctx, const int32_t *rows_d, int b,
                                      const int32_t *next_rows_d, int next_b, float clip_lo,
                                      float clip_hi, float entropy_coef, float inv_b,
                                      float inv_ba, float *grad_d, float *loss_d, float *m_d,
                                      float *v_d, const float *sched_d, float neg_step_actor,
                                      float neg_step_critic, float bc2_sqrt,
                                      float one_minus_beta1, float beta2, float one_minus_beta2,
                                      float eps, int flags, void *stream) {
  if (int rc = check_ctx(ctx)) return rc;
  PPO_REQUIRE(fused_active(ctx) && ctx->frec && ctx->frec_rows > 0,
              "ppo_update_step_staged: no staged records (ppo_stage_records first)");
  PPO_REQUIRE(rows_d && grad_d && loss_d && m_d && v_d, "ppo_update_step_staged: null buffer");
  PPO_REQUIRE(b > 0 && b <= ctx->cfg.max_rows && next_b >= 0 && next_b <= ctx->cfg.max_rows &&
                  (next_b == 0) == (next_rows_d == nullptr),
              "ppo_update_step_staged: b=%d next_b=%d (max_rows %d)", b, next_b,
              ctx->cfg.max_rows);
  PPO_REQUIRE((flags & ~(PPO_STAGED_WEIGHTS_CURRENT | PPO_STAGED_ROWS_GATHERED)) == 0,
              "ppo_update_step_staged: flags %d", flags);
  hipStream_t st = as_stream(stream);
  TimingScope timing_scope(ctx->tim);
  const bool gathered = (flags & PPO_STAGED_ROWS_GATHERED) && gathered_holds(ctx, rows_d, b);
  const bool current = flags & PPO_STAGED_WEIGHTS_CURRENT;
  FusedArgs q = fused_args(ctx, nullptr, nullptr, nullptr, nullptr, nullptr, rows_d, b, nullptr,
                           LossCoef{clip_lo, clip_hi, entropy_coef, inv_b, inv_ba}, true, !current);
  if ((!gathered && !q.direct) || !current) {
    FusedArgs p = q;
    p.b = (gathered || q.direct) ? 0 : b;
    if (int rc = fused_prep(ctx, p, st)) return rc;
    if (p.b > 0) note_gathered(ctx, rows_d, b);
  }
  // tail: slab reduction + Adam + weight images, and the next minibatch's row gather
  ReduceArgs r;
  if (int rc = fused_reduce_args(ctx, q, grad_d, loss_d, r)) return rc;
  TailArgs t{};
  t.a = adam_pack_args(ctx, grad_d, m_d, v_d, sched_d, neg_step_actor, neg_step_critic, bc2_sqrt,
                       one_minus_beta1, beta2, one_minus_beta2, eps);
  t.rows = next_rows_d;
  t.rec = ctx->frec;
  t.n_rec = ctx->frec_rows;
  t.xb = ctx->fxb;
  t.srow = ctx->fsrow;
  t.b = q.direct ? 0 : next_b;  // direct: the next fused launch reads its rows itself
  t.reduce = true;
  t.slabs = ctx->fslabs;  // the layout fused_reduce_args describes segment by segment
  t.slab_stride = ctx->total_params;
  t.nsplit = q.G;
  if (int rc = fused_forward_backward(ctx, q, st)) {
    note_gathered(ctx, nullptr, 0);
    return rc;
  }
  const double P = static_cast<double>(ctx->total_params), H = ctx->fused_hidden;
  const TimRec rec{KC_REDUCE, "step_tail_kernel", static_cast<double>(q.G) * P,
                   4.0 * (q.G + 1.0) * P + 24.0 * P + 2.0 * 2.0 * H * (q.din + 2.0 * H) +
                       static_cast<double>(t.b) * (4.0 + 2.0 * kRecordBytes)};
  if (int rc = step_tail_launch(r, t, rec, st)) {
    note_gathered(ctx, nullptr, 0);
    return rc;
  }
  if (t.b > 0) note_gathered(ctx, next_rows_d, t.b);
  return 0;
}

extern "C" int ppo_observe_act(ppo_ctx *ctx, double *window_d, const double *obs_d,
                               const uint8_t *reset_d, int all_reset, const int32_t *bounds,
                               int n_bounds, int normalize, float *state_d, int n,
                               const float *eps_d, uint64_t seed, uint64_t offset,
                               float *action_d, float *logp_d, float *value_d, float *mean_d,
                               void *stream) {
  if (int rc = check_ctx(ctx)) return rc;
  const int o = ctx->cfg.obs_dim, w = ctx->cfg.window;
  PPO_REQUIRE(window_d && state_d && n > 0, "ppo_observe_act: null window/state or n <= 0");
  PPO_REQUIRE(n <= ctx->cfg.max_rows, "ppo_observe_act: n=%d exceeds max_rows=%d", n,
              ctx->cfg.max_rows);
  PPO_REQUIRE(n_bounds >= 0 && n_bounds < 16, "ppo_observe_act: too many slices (%d)", n_bounds);
  PolicySlices tab{};
  tab.count = normalize ? n_bounds : 0;
  for (int i = 0; i <= n_bounds && normalize; ++i) {
    PPO_REQUIRE(bounds != nullptr, "ppo_observe_act: null bounds");
    PPO_REQUIRE(bounds[i] >= 0 && bounds[i] <= o && (i == 0 || bounds[i] >= bounds[i - 1]),
                "ppo_observe_act: bounds must be ascending within [0, O]");
    tab.edge[i] = bounds[i];
  }
  if (!fused_active(ctx) && wide_active(ctx) && wide_observe_ok(ctx, tab.count)) {
    // wide path: window push + standardisation + bf16 operand rows in one launch, then the GEMMs
    TimingScope timing_scope(ctx->tim);
    if (int rc = wide_observe(ctx, window_d, obs_d, reset_d, all_reset, tab, normalize, state_d, n,
                              as_stream(stream)))
      return rc;
    return wide_policy_step(ctx, state_d, n, eps_d, seed, offset, action_d, logp_d, value_d,
                            mean_d, false, as_stream(stream), true);
  }
  if (!fused_active(ctx) || w > kPolicyMaxWindow) {  // layered: A1 kernels, then GEMM policy step
    if (obs_d) {
      int rc = ppo_obs_window_push(window_d, obs_d, 1, reset_d, all_reset, n, o, w, stream);
      if (rc) return rc;
    }
    if (int rc = ppo_obs_normalize(window_d, state_d, n, o, w, bounds, n_bounds, normalize, stream))
      return rc;
    if (wide_active(ctx)) {  // the weight images are current (ppo_pack_weights before the rollout)
      TimingScope timing_scope(ctx->tim);
      return wide_policy_step(ctx, state_d, n, eps_d, seed, offset, action_d, logp_d, value_d,
                              mean_d, false, as_stream(stream));
    }
    return ppo_policy_step(ctx, state_d, n, eps_d, seed, offset, action_d, logp_d, value_d,
                           mean_d, stream);
  }
  TimingScope timing_scope(ctx->tim);
  PolicyFusedArgs q{};
  fused_nets(ctx, q.net);
  q.logstd = ctx->params + ctx->net[0].logstd_off;
  q.n = n;
  q.obs_dim = o;
  q.window = w;
  q.act_dim = ctx->cfg.act_dim;
  q.act = ctx->cfg.activation;
  q.hidden = ctx->fused_hidden;
  q.omv = ctx->cfg.output_max_value;
  q.window_d = window_d;
  q.obs_d = obs_d;
  q.reset_d = reset_d;
  q.all_reset = all_reset;
  q.tab = tab;
  q.normalize = normalize;
  q.state_d = state_d;
  q.do_actor = (action_d || logp_d || mean_d) ? 1 : 0;
  q.do_critic = value_d ? 1 : 0;
  q.eps = eps_d;
  q.seed = seed;
  q.offset = offset;
  q.offset_base = ctx->rng_counter;
  q.stamps = ctx->fstamp_on ? ctx->fstamps : nullptr;
  if (q.stamps) ctx->fstamp_g = 128;
  q.action = action_d;
  q.logp = logp_d;
  q.value = value_d;
  q.mean = mean_d;
  const double H = ctx->fused_hidden, A = ctx->cfg.act_dim, din = o * w;
  const double fl = 2.0 * n * ((q.do_actor ? din * H + H * H + A * H : 0.0) +
                               (q.do_critic ? din * H + H * H + H : 0.0));
  const double by = static_cast<double>(n) *
                    (8.0 * o * w * (obs_d ? 2.0 : 1.0) + (obs_d ? 8.0 * o : 0.0) + 4.0 * din +
                     (eps_d ? 4.0 * A : 0.0) + (action_d ? 4.0 * A : 0.0) + (mean_d ? 4.0 * A : 0.0) +
                     (logp_d ? 4.0 : 0.0) + (value_d ? 4.0 : 0.0));
  const TimRec rec{KC_POLICY_HEAD,
                   tim_active() ? intern_name("policy_fused_kernel<%d, %d, %d, false>", ctx->fused_hidden, q.act,
                                             q.act_dim <= 2 ? 2 : q.act_dim <= 4 ? 4 : q.act_dim <= 6 ? 6 : 8)
                                : nullptr,
                   fl, by};
  return policy_fused_launch(q, rec, as_stream(stream));
}

// the shapes the persistent rollout kernels are compiled for
static int rollout_ctx_ok(const ppo_ctx *ctx, const char *who) {
  PPO_REQUIRE(fused_active(ctx), "%s: needs the fused bf16 path (ppo_ctx_fused_active)", who);
  PPO_REQUIRE(ctx->cfg.window == 1 && ctx->cfg.obs_dim <= kFusedKX && ctx->fused_hidden == 256,
              "%s: needs W = 1, O <= %d and hidden width 256 (W = %d, O = %d, H = %d)", who,
              kFusedKX, ctx->cfg.window, ctx->cfg.obs_dim, ctx->fused_hidden);
  return 0;
}

extern "C" int ppo_rollout_synthetic(ppo_ctx *ctx, const float *base_obs_d,
                                     const float *base_reward_d, const uint8_t *base_term_d,
                                     int t_len, int n, double *window_d, const int32_t *bounds,
                                     int n_bounds, int normalize, float *states_d,
                                     const float *noise_d, uint64_t seed, uint64_t offset,
                                     float *actions_d, float *logp_d, double *reward_d,
                                     uint8_t *terminated_d, void *stream) {
  (void)seed;    // carried for symmetry with ppo_observe_act: the kernel reads the pre-drawn noise
  (void)offset;
  if (int rc = check_ctx(ctx)) return rc;
  if (int rc = rollout_ctx_ok(ctx, "ppo_rollout_synthetic")) return rc;
  PPO_REQUIRE(base_obs_d && base_reward_d && base_term_d && window_d && states_d && noise_d &&
                  actions_d && logp_d && reward_d && terminated_d,
              "ppo_rollout_synthetic: null buffer");
  PPO_REQUIRE(n > 0 && t_len > 0, "ppo_rollout_synthetic: bad shape n=%d t=%d", n, t_len);
  PPO_REQUIRE(n <= ctx->cfg.max_rows, "ppo_rollout_synthetic: n=%d exceeds max_rows=%d", n,
              ctx->cfg.max_rows);
  PPO_REQUIRE(n_bounds >= 0 && n_bounds < 16, "ppo_rollout_synthetic: too many slices (%d)",
              n_bounds);
  const int o = ctx->cfg.obs_dim;
  PolicySlices tab{};
  tab.count = normalize ? n_bounds : 0;
  for (int i = 0; i <= n_bounds && normalize; ++i) {
    PPO_REQUIRE(bounds != nullptr, "ppo_rollout_synthetic: null bounds");
    PPO_REQUIRE(bounds[i] >= 0 && bounds[i] <= o && (i == 0 || bounds[i] >= bounds[i - 1]),
                "ppo_rollout_synthetic: bounds must be ascending within [0, O]");
    tab.edge[i] = bounds[i];
  }
  TimingScope timing_scope(ctx->tim);
  FusedNet nets[2];
  fused_nets(ctx, nets);
  RolloutArgs q{};
  q.net = nets[0];
  q.logstd = ctx->params + ctx->net[0].logstd_off;
  q.n = n;
  q.obs_dim = o;
  q.act_dim = ctx->cfg.act_dim;
  q.act = ctx->cfg.activation;
  q.hidden = ctx->fused_hidden;
  q.t_len = t_len;
  q.omv = ctx->cfg.output_max_value;
  q.window_d = window_d;
  q.base_obs = base_obs_d;
  q.base_reward = base_reward_d;
  q.base_term = base_term_d;
  q.tab = tab;
  q.normalize = normalize;
  q.noise = noise_d;
  q.states = states_d;
  q.actions = actions_d;
  q.logp = logp_d;
  q.reward = reward_d;
  q.terminated = terminated_d;
  q.stamps = (ctx->fstamp_on && q.act == PPO_ACT_RELU) ? ctx->fstamps : nullptr;
  if (q.stamps) ctx->fstamp_g = 128;
  const double H = ctx->fused_hidden, A = q.act_dim, rows = static_cast<double>(n) * t_len;
  const TimRec rec{KC_POLICY_HEAD,
                   tim_active() ? intern_name("rollout_persistent_kernel<%d, %d>", ctx->fused_hidden, q.act)
                                : nullptr,
                   2.0 * rows * (o * H + H * H + A * H),
                   rows * (8.0 * o + 8.0 * A + 4.0 + 4.0 + 1.0 + 8.0 + 1.0) + 12.0 * n * o};
  return rollout_persistent_launch(q, rec, as_stream(stream));
}

extern "C" int ppo_value_batch(ppo_ctx *ctx, const float *states_d, int64_t rows, float *values_d,
                               void *stream) {
  if (int rc = check_ctx(ctx)) return rc;
  if (int rc = rollout_ctx_ok(ctx, "ppo_value_batch")) return rc;
  PPO_REQUIRE(states_d && values_d, "ppo_value_batch: null buffer");
  PPO_REQUIRE(rows > 0, "ppo_value_batch: rows=%lld must be positive", static_cast<long long>(rows));
  int num_cu = 0;
  PPO_HIP_TRY(hipDeviceGetAttribute(&num_cu, hipDeviceAttributeMultiprocessorCount, ctx->device));
  TimingScope timing_scope(ctx->tim);
  FusedNet nets[2];
  fused_nets(ctx, nets);
  ValueBatchArgs q{};
  q.net = nets[1];
  q.obs_dim = ctx->cfg.obs_dim;
  q.act = ctx->cfg.activation;
  q.hidden = ctx->fused_hidden;
  q.rows = rows;
  q.states = states_d;
  q.values = values_d;
  const double H = ctx->fused_hidden, o = q.obs_dim;
  const TimRec rec{KC_POLICY_HEAD,
                   tim_active() ? intern_name("value_batch_kernel<%d, %d>", ctx->fused_hidden, q.act)
                                : nullptr,
                   2.0 * rows * (o * H + H * H + H), rows * (4.0 * o + 4.0)};
  return value_batch_launch(q, num_cu, rec, as_stream(stream));
}

extern "C" int ppo_minibatch_grad(ppo_ctx *ctx, const float *states_d, const float *actions_d,
                                  const float *old_logp_d, const float *adv_d,
                                  const float *vtarget_d, const int32_t *rows_d, int b,
                                  const int32_t *count_d, float clip_lo, float clip_hi,
                                  float entropy_coef, float inv_b, float inv_ba, float *grad_d,
                                  float *loss_d, void *stream) {
  if (int rc = check_ctx(ctx)) return rc;
  PPO_REQUIRE(states_d && actions_d && old_logp_d && adv_d && vtarget_d && rows_d && grad_d,
              "ppo_minibatch_grad: null buffer");
  PPO_REQUIRE(b > 0 && b <= ctx->cfg.max_rows, "ppo_minibatch_grad: b=%d outside [1, max_rows=%d]",
              b, ctx->cfg.max_rows);
  const LossCoef coef{clip_lo, clip_hi, entropy_coef, inv_b, inv_ba};
  hipStream_t st = as_stream(stream);
  TimingScope timing_scope(ctx->tim);
  if (fused_active(ctx))
    return fused_minibatch_grad(ctx, states_d, actions_d, old_logp_d, adv_d, vtarget_d, rows_d, b,
                                count_d, coef, grad_d, loss_d, st);
  if (wide_active(ctx))
    return wide_minibatch_grad(ctx, states_d, actions_d, old_logp_d, adv_d, vtarget_d, rows_d, b,
                               count_d, coef, grad_d, loss_d, st);
  return layered_minibatch_grad(ctx, states_d, actions_d, old_logp_d, adv_d, vtarget_d, rows_d, b,
                                count_d, coef, grad_d, loss_d, st);
}

extern "C" int ppo_ctx_phase_stamps(ppo_ctx *ctx, int enable, uint64_t *host_out, int max_values) {
  PPO_REQUIRE(ctx != nullptr, "ppo_ctx_phase_stamps: null ctx");
  PPO_REQUIRE(ctx->fused_ok, "ppo_ctx_phase_stamps: network shape has no fused kernel");
  PPO_HIP_TRY(hipSetDevice(ctx->device));
  const int n = 2 * kFusedMaxWG * kStampSlots;
  if (enable) {
    if (!ctx->fstamps) PPO_HIP_TRY(hipMalloc(&ctx->fstamps, sizeof(uint64_t) * n));
    PPO_HIP_TRY(hipMemset(ctx->fstamps, 0, sizeof(uint64_t) * n));
    ctx->fstamp_on = 1;
    return 0;
  }
  ctx->fstamp_on = 0;
  if (!ctx->fstamps) return 0;
  PPO_HIP_TRY(hipDeviceSynchronize());
  const int got = 2 * ctx->fstamp_g * kStampSlots;
  if (host_out && max_values > 0)
    PPO_HIP_TRY(hipMemcpy(host_out, ctx->fstamps, sizeof(uint64_t) * std::min(got, max_values),
                          hipMemcpyDeviceToHost));
  return got;
}

extern "C" int ppo_ctx_fused_constants(ppo_ctx *ctx, int net, void *host_out, int64_t bytes) {
  PPO_REQUIRE(ctx != nullptr, "ppo_ctx_fused_constants: null ctx");
  PPO_REQUIRE(ctx->fused_ok, "ppo_ctx_fused_constants: network shape has no fused kernel");
  const int64_t size = fused_const_bytes(ctx->fused_hidden);
  if (!host_out) return static_cast<int>(size);
  PPO_REQUIRE((net == 0 || net == 1) && bytes >= 0 && bytes <= size,
              "ppo_ctx_fused_constants: net %d, %lld of %lld bytes", net,
              static_cast<long long>(bytes), static_cast<long long>(size));
  PPO_HIP_TRY(hipSetDevice(ctx->device));
  PPO_HIP_TRY(hipDeviceSynchronize());
  PPO_HIP_TRY(hipMemcpy(host_out, ctx->fconst[net], bytes, hipMemcpyDeviceToHost));
  return static_cast<int>(size);
}

extern "C" int ppo_ctx_set_precision(ppo_ctx *ctx, int prec) {
  PPO_REQUIRE(ctx != nullptr, "ppo_ctx_set_precision: null ctx");
  PPO_REQUIRE(prec == PPO_PREC_F32 || prec == PPO_PREC_BF16,
              "ppo_ctx_set_precision: unknown precision %d", prec);
  ctx->prec = prec;
  if (prec == PPO_PREC_BF16)  // the wide path's workspace, for the shapes it covers
    if (int rc = wide_alloc(ctx)) return rc;
  return 0;
}

extern "C" int ppo_ctx_loss_entropy_share(ppo_ctx *ctx, float share) {
  PPO_REQUIRE(ctx != nullptr, "ppo_ctx_loss_entropy_share: null ctx");
  ctx->ent_log_share = share;
  return 0;
}

extern "C" int ppo_ctx_fused_direct(ppo_ctx *ctx, int enable) {
  PPO_REQUIRE(ctx != nullptr, "ppo_ctx_fused_direct: null ctx");
  if (enable < 0) return ctx->fdirect ? 1 : 0;
  ctx->fdirect = enable != 0;
  note_gathered(ctx, nullptr, 0);
  return 0;
}

extern "C" int ppo_ctx_set_rng_counter(ppo_ctx *ctx, const uint64_t *counter_d) {
  PPO_REQUIRE(ctx != nullptr, "ppo_ctx_set_rng_counter: null ctx");
  ctx->rng_counter = counter_d;
  return 0;
}

extern "C" int ppo_ctx_timing(ppo_ctx *ctx, int enable, int capacity) {
  PPO_REQUIRE(ctx != nullptr, "ppo_ctx_timing: null ctx");
  return timing_enable(ctx->tim, enable, capacity);
}

extern "C" int ppo_ctx_timing_read(ppo_ctx *ctx, int kclass, double *total_ms, int64_t *launches,
                                   double *flops, double *bytes) {
  PPO_REQUIRE(ctx != nullptr, "ppo_ctx_timing_read: null ctx");
  return timing_read_class(ctx->tim, kclass, total_ms, launches, flops, bytes);
}

extern "C" int ppo_ctx_timing_kernel(ppo_ctx *ctx, int index, const char **name, int *kclass,
                                     double *total_ms, int64_t *launches, double *flops,
                                     double *bytes) {
  PPO_REQUIRE(ctx != nullptr, "ppo_ctx_timing_kernel: null ctx");
  return timing_read_kernel(ctx->tim, index, name, kclass, total_ms, launches, flops, bytes);
}
