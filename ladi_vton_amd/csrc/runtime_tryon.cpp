// Native try-on pipeline: steps 4b-11 of StableDiffusionTryOnePipeline.__call__
// (src/vto_pipelines/tryon_pipe.py:630-753) with the denoising step hipGraph-captured.
#include "runtime.h"
#include <stdexcept>
#include <cstring>
#include <cmath>

namespace ladi {

#define HIP_OK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) throw std::runtime_error(std::string(#x) + ": " + hipGetErrorString(e_)); } while (0)
// outside a try block of run(): report and return
#define HIP_OK_RC(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { set_error(std::string("tryon: " #x ": ") + hipGetErrorString(e_)); return -100; } } while (0)

void GraphTable::clear() {
    for (auto& ge : e) if (ge) { (void)hipGraphExecDestroy(ge); ge = nullptr; }
    for (auto& gr : g) if (gr) { (void)hipGraphDestroy(gr); gr = nullptr; }
}

void GraphTable::capture(int f, hipStream_t st, const std::function<void()>& fn) {
    hipGraph_t& gr = g[f];
    hipGraphExec_t& ge = e[f];
    if (gr) { (void)hipGraphDestroy(gr); gr = nullptr; }
    HIP_OK(hipStreamBeginCapture(st, hipStreamCaptureModeRelaxed));
    try { fn(); } catch (...) { hipGraph_t x = nullptr; (void)hipStreamEndCapture(st, &x); if (x) (void)hipGraphDestroy(x); throw; }
    HIP_OK(hipStreamEndCapture(st, &gr));
    HIP_OK(hipGraphInstantiate(&ge, gr, nullptr, nullptr, 0));
    ++captures;
}

TryOn::~TryOn() {
    graphs.clear();
    if (fcache) (void)hipFree(fcache);
    if (stats) (void)hipFree(stats);
    if (step_noise_buf) (void)hipFree(step_noise_buf);
    if (ip_buf) (void)hipFree(ip_buf);
    for (auto& e : ev) if (e) (void)hipEventDestroy(e);
    if (ev_in) (void)hipEventDestroy(ev_in);
    if (ev_out) (void)hipEventDestroy(ev_out);
    if (own_stream) (void)hipStreamDestroy(own_stream);
}

int TryOn::stage_ms(float out[3]) {
    if (!ev_valid) return -1;
    for (int i = 0; i < 3; ++i) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, ev[i], ev[i + 1]) != hipSuccess) return -2;
        out[i] = ms;
    }
    return 0;
}

// ------------------------------------------------------------------------------------------------ the evaluation plan (host only)
// the run is CFG-shaped if ANY evaluation's scale is > 1; a set schedule replaces the scalar
static bool cfg_shaped(float guidance, const std::vector<float>& g_sched) {
    if (g_sched.empty()) return guidance > 1.0f;
    for (float g : g_sched) if (g > 1.0f) return true;
    return false;
}

static int refuse(EvalPlan& p, int rc, const std::string& msg) { p.rc = rc; p.error = msg; return rc; }
static int wrong_length(EvalPlan& p, int rc, const char* what, size_t have, int evals, int first_step, int steps) {
    return refuse(p, rc, std::string("tryon: the ") + what + " has " + std::to_string(have) + " entries, this run has " + std::to_string(evals) +
                  " evaluations (PNDM: steps + 1" + (first_step ? "; the run starts at step " + std::to_string(first_step) + " of " +
                  std::to_string(steps) : std::string()) + ")");
}

int plan_evals(EvalPlan& p, int evals, int first_step, int steps, float guidance, const std::vector<float>& g_sched, float phi,
               const std::vector<float>& pag_sched, const std::vector<unsigned char>& fc_plan, const SagPlan* sag) {
    p = EvalPlan();
    p.sag_on = sag && sag->scale != 0.f;
    const bool has_sched = !g_sched.empty();
    p.cfg = cfg_shaped(guidance, g_sched);
    p.guided = p.cfg && (has_sched || phi > 0.f);
    p.use_factor = p.guided && phi > 0.f;
    p.ng = p.cfg ? 2 : 1;
    if (has_sched && (int)g_sched.size() != evals) return wrong_length(p, -9, "guidance schedule", g_sched.size(), evals, first_step, steps);
    // perturbed-attention guidance: one scale per evaluation
    if (!pag_sched.empty() && (int)pag_sched.size() != evals) return wrong_length(p, -9, "PAG table", pag_sched.size(), evals, first_step, steps);
    for (float s : pag_sched) p.pag_on = p.pag_on || s > 0.f;
    if (p.pag_on && !fc_plan.empty())
        return refuse(p, TRYON_PAG_WITH_CACHE, "tryon: perturbed-attention guidance together with a feature-cache plan is not supported (the cache's "
                      "group promotion has no third group): clear one of ladi_tryon_set_pag / ladi_tryon_set_feature_cache");
    // self-attention guidance: what it cannot run with.  A feature-cache plan counts whatever its flags say (as for PAG)
    if (p.sag_on) {
        const char* off = ": set ladi_tryon_set_sag(t, 0) or ";
        if (!fc_plan.empty())
            return refuse(p, TRYON_SAG_WITH_CACHE, std::string("tryon: self-attention guidance together with a feature-cache plan is not supported (a shallow "
                          "evaluation does not run the mid block, whose attention map SAG reads)") + off + "clear ladi_tryon_set_feature_cache");
        if (p.pag_on)
            return refuse(p, TRYON_SAG_WITH_PAG, std::string("tryon: self-attention guidance together with a positive PAG scale is not supported (both "
                          "claim the sample group behind the conditional one)") + off + "clear ladi_tryon_set_pag");
        if (sag->mid_merges)
            return refuse(p, TRYON_SAG_TOME_MID, std::string("tryon: self-attention guidance with token merging in the mid block is not supported (the "
                          "map would have merged tokens)") + off + "merge on the outer levels only");
        const int kind = decode_sched_code(sag->scheduler).kind;
        if (kind == SCHED_LMS || kind == SCHED_EULER || kind == SCHED_EULER_A)
            return refuse(p, TRYON_SAG_SCHEDULER, std::string("tryon: self-attention guidance does not run with the sigma-space schedulers (Euler, "
                          "Euler-ancestral, LMS: their model input is rescaled, and pred_x0 / add_noise do not describe them)") + off +
                          "use DDIM, PNDM, DPM-Solver++, LCM or TCD");
        if (sag->h < 5 || sag->w < 5)
            return refuse(p, TRYON_SAG_SMALL, "tryon: self-attention guidance needs latents of at least 5 x 5 (the blur's 4-pixel reflect padding), got " +
                          std::to_string(sag->h) + " x " + std::to_string(sag->w) + off + "run a larger image");
    }
    if (!fc_plan.empty()) {
        if ((int)fc_plan.size() != evals) return wrong_length(p, -10, "feature-cache plan", fc_plan.size(), evals, first_step, steps);
        if (!fc_plan[0]) return refuse(p, -10, "tryon: the feature-cache plan must start with a whole evaluation (flag 0 = 1)");
    }
    p.groups = p.ng + (p.pag_on ? 1 : 0);
    p.gtab = has_sched ? g_sched : std::vector<float>(evals, guidance);
    p.form.resize(evals);
    // deep-feature cache plan: one flag per evaluation, 1 = whole forward.  The one promotion: a shallow evaluation over all 2B samples needs a
    // cache whose two halves were written by the same whole evaluation, so after a whole evaluation that ran cond-only (rows [B, 2B) only) it
    // runs whole
    bool halves_differ = false;      // the most recent whole evaluation refreshed the conditional rows only
    for (int i = 0; i < evals; ++i) {
        // cond-only: scale <= 1 in a guided run (no unconditional half, as do_classifier_free_guidance of a whole run)
        const bool cond = p.guided && !(p.gtab[i] > 1.0f);
        bool whole = fc_plan.empty() || fc_plan[i];
        if (!whole && p.cfg && !cond && halves_differ) whole = true;
        if (whole) halves_differ = p.cfg && cond;
        p.fc_on = p.fc_on || !whole;
        p.form[i] = (unsigned char)((cond ? 1 : 0) | (whole ? 0 : 2) | (p.pag_on && pag_sched[i] > 0.f ? 4 : 0));
        p.has_form[p.form[i]] = true;
    }
    return 0;
}

// ------------------------------------------------------------------------------------------------ one run
// what the stages of one run() share: the arguments, the host plan, and the buffers of the current pass (dry, then real)
struct TryOn::Run {
    const TryOnInputs& in; void* images_out; int images_u8; float* latents_out; hipStream_t user_st, st;
    int B = 0, H = 0, W = 0, h = 0, w = 0, hw = 0, pose_ch = 0, L = 0, D = 0, first_step = 0, evals = 0, n = 0, rows = 0;
    bool has_cloth = false, keep_lat = false, keep_pix = false, use_step_noise = false; size_t step_noise_bytes = 0;
    EvalPlan plan;
    std::vector<float> ac, keep_tab, sag_tab; std::vector<double> timesteps; std::vector<StepTable> table; SchedInfo sinfo;
    Ctx c;
    h16 *ehs, *mask_bin, *mask2, *mask4, *mask8, *pose_lat;
    float *cloth_lat, *masked_lat, *latents, *cur_sample, *ets, *keep_x0, *keep_noise, *keep_mask;
    Act unet_in, skips[5];
    // -5 / -6: time embedding / context failed in the real pass (the error is set; the streams are joined like on success); the callback's
    int rc = 0, cb_rc = 0, cb_eval = -1;
};

int TryOn::run(const TryOnInputs& in, void* images_out, int images_u8, float* latents_out, hipStream_t user_st) {
    if (!unet || !vae) { set_error("tryon: unet and vae are required"); return -1; }
    Run r{in, images_out, images_u8, latents_out, user_st, user_st};
    if (int rc = enter(r)) return rc;
    if (int rc = plan(r)) return rc;
    if (int rc = grow_tables(r)) return rc;
    hipStream_t st = r.st;
    try {
        lanes.configure(r.n, lanes_override > 0 && (r.n % lanes_override) == 0 ? lanes_override : 0);
        for (int pass = 0; pass < 2; ++pass) {
            arena.dry = (pass == 0);
            arena.off = 0;
            r.c = Ctx(); r.c.st = st; r.c.ar = &arena; r.c.stats = stats; r.c.stats_cap = stats_cap; r.c.sk_cnt = sk_cnt;
            if (pass == 1) upload_tables(r);
            if (!r.rc) encode(r);
            if (r.rc) break;
            denoise(r);
            if (r.cb_rc) {
                // the handle stays usable: the next run re-arms the step counter and the arrival ticket (upload_tables)
                set_error("tryon: the step callback returned " + std::to_string(r.cb_rc) + " after evaluation " + std::to_string(r.cb_eval) +
                          ": run aborted");
                ev_valid = false;
                HIP_OK(hipEventRecord(ev_out, st));
                HIP_OK(hipStreamWaitEvent(user_st, ev_out, 0));
                return TRYON_CALLBACK_ABORT;
            }
            decode(r);
            if (pass == 0) {
                lanes.commit_plan();
                commit_plan(arena, r.c.stats_peak, &stats, &stats_cap);
            }
        }
        HIP_OK(hipEventRecord(ev_out, st));
        HIP_OK(hipStreamWaitEvent(user_st, ev_out, 0));
    } catch (const std::exception& e) {
        set_error(std::string("tryon: ") + e.what());
        (void)hipEventRecord(ev_out, st);
        (void)hipStreamWaitEvent(user_st, ev_out, 0);
        return -100;
    }
    return r.rc;
}

int TryOn::enter(Run& r) {
    try {
        if (!own_stream) {
            HIP_OK(hipStreamCreateWithFlags(&own_stream, hipStreamNonBlocking));
            HIP_OK(hipEventCreateWithFlags(&ev_in, hipEventDisableTiming));
            HIP_OK(hipEventCreateWithFlags(&ev_out, hipEventDisableTiming));
        }
        HIP_OK(hipEventRecord(ev_in, r.user_st));
        HIP_OK(hipStreamWaitEvent(own_stream, ev_in, 0));
        r.st = own_stream;
    } catch (const std::exception& e) { set_error(std::string("tryon: ") + e.what()); return -100; }
    try {
        if (vae->poll_overflow()) {      // the PREVIOUS run's decode left the fp16 range: its images are invalid and nobody asked (ladi_tryon_poll_overflow)
            set_error("tryon: the previous run's VAE decode overflowed the fp16 range (non-finite GroupNorm statistics) at range shift " + std::to_string(vae->last_shift) +
                      "; its images are invalid -- re-submit that batch (the automatic shift is now " + std::to_string(vae->guard_shift()) + ")");
            (void)hipEventRecord(ev_out, r.st); (void)hipStreamWaitEvent(r.user_st, ev_out, 0);
            return -101;
        }
    } catch (const std::exception& e) { set_error(std::string("tryon: ") + e.what()); return -100; }
    return 0;
}

int TryOn::plan(Run& r) {
    const TryOnInputs& in = r.in;
    r.B = in.batch; r.H = in.height; r.W = in.width;
    if (r.H % 8 || r.W % 8) { set_error("height and width must be divisible by 8"); return -2; }
    r.h = r.H / 8; r.w = r.W / 8; r.hw = r.h * r.w;
    r.has_cloth = in.warped_cloth != nullptr;
    r.pose_ch = in.pose_channels;
    if (9 + r.pose_ch + (r.has_cloth ? 4 : 0) != unet->cfg.in_channels) { set_error("tryon: UNet in_channels does not match 9 + pose + cloth channels"); return -3; }
    r.L = in.L; r.D = unet->cfg.cross_dim;
    if (ip_pos && !unet->ip_loaded) {
        set_error("tryon: image embeddings are set (ladi_tryon_set_ip_adapter) but the UNet has no IP-Adapter loaded (ladi_unet_ip_adapter_load)");
        return TRYON_IP_NO_ADAPTER;
    }
    if (ip_pos && (ip_T > 0) != (unet->ip_resampler != nullptr)) {
        set_error(ip_T > 0 ? "tryon: hidden states are set (ladi_tryon_set_ip_adapter_seq) but the loaded IP-Adapter is a plain adapter, which takes one "
                             "embedding per image (ladi_tryon_set_ip_adapter)"
                           : "tryon: image embeddings are set (ladi_tryon_set_ip_adapter) but the loaded IP-Adapter is a Plus adapter, which takes hidden "
                             "states (ladi_tryon_set_ip_adapter_seq)");
        return TRYON_IP_ADAPTER_KIND;
    }
    if (cfg_shaped(in.guidance, g_sched) && !in.negative_prompt_embeds) { set_error("tryon: negative_prompt_embeds required when guidance_scale > 1"); return -4; }
    // ---- scheduler tables (host)
    if (in.alphas_cumprod) r.ac.assign(in.alphas_cumprod, in.alphas_cumprod + 1000); else default_alphas_cumprod(r.ac);
    // a set init (ladi_tryon_set_init) starts the run at step first_step of the schedule: the tables below are the tail's, indexed from 0
    r.first_step = (init_src && init_first > 0) ? init_first : 0;
    build_step_table(in.scheduler, in.steps, r.ac.data(), in.cloth_zero_from, r.timesteps, r.table, &r.sinfo, eta, r.first_step);
    r.evals = (int)r.timesteps.size();
    SagPlan sp; sp.scale = sag_scale; sp.scheduler = in.scheduler; sp.h = r.h; sp.w = r.w;
    for (int b : unet->tome_blocks()) sp.mid_merges = sp.mid_merges || b == unet->mid_bit;
    if (plan_evals(r.plan, r.evals, r.first_step, in.steps, in.guidance, g_sched, phi, pag_sched, fc_plan, &sp)) { set_error(r.plan.error); return r.plan.rc; }
    r.n = r.plan.groups * r.B;
    r.rows = r.n + (r.plan.sag_on ? r.B : 0);     // SAG: the degraded input's rows of unet_in and eps; the context stays r.n samples
    // preserve-unmasked: the blend's coefficients per evaluation, float64 on the host like the step table
    r.keep_lat = (preserve_mode & 1) != 0; r.keep_pix = (preserve_mode & 2) != 0;
    if (r.keep_lat) keep_coeffs_of(in.scheduler, r.timesteps, r.sinfo, r.ac.data(), r.first_step, r.keep_tab);
    // self-attention guidance: sqrt(a), sqrt(1 - a) at every evaluation's (integer) timestep and the model-input scale, which is 1 for every
    // scheduler SAG runs with; float64 on the host like the step table
    if (r.plan.sag_on) {
        r.sag_tab.assign((size_t)r.evals * 4, 0.f);
        for (int i = 0; i < r.evals; ++i) {
            long t = std::lround(r.timesteps[i]);
            t = t < 0 ? 0 : t > 999 ? 999 : t;
            const double a = (double)r.ac[(size_t)t];
            r.sag_tab[4 * i] = (float)std::sqrt(a); r.sag_tab[4 * i + 1] = (float)std::sqrt(1.0 - a); r.sag_tab[4 * i + 2] = 1.f;
        }
    }
    last_shallow = 0;
    last_evals = r.evals;
    last_cond_only = 0;      // counted in denoise(), where an evaluation over B samples is actually launched
    return 0;
}

int TryOn::grow_tables(Run& r) {
    const EvalPlan& p = r.plan;
    const int evals = r.evals, B = r.B;
    if (!d_step) d_step = reinterpret_cast<int*>(pool.alloc(256));
    if (!sk_cnt) { sk_cnt = reinterpret_cast<int*>(pool.alloc(1024 * sizeof(int))); HIP_OK(hipMemset(sk_cnt, 0, 1024 * sizeof(int))); }
    if (evals > table_cap) { d_table = reinterpret_cast<StepTable*>(pool.alloc((size_t)evals * sizeof(StepTable))); table_cap = evals; }
    if (p.guided && evals > gtab_cap) { d_gtab = reinterpret_cast<float*>(pool.alloc((size_t)evals * sizeof(float))); gtab_cap = evals; }
    if (p.pag_on && evals > pag_cap) { d_pag = reinterpret_cast<float*>(pool.alloc((size_t)evals * sizeof(float))); pag_cap = evals; }
    if (p.sag_on && !d_sag) d_sag = reinterpret_cast<float*>(pool.alloc(256));
    if (p.sag_on && evals > sag_tab_cap) { d_sag_tab = reinterpret_cast<float*>(pool.alloc((size_t)evals * 4 * sizeof(float))); sag_tab_cap = evals; }
    if (p.use_factor && B > factor_cap) { d_factor = reinterpret_cast<float*>(pool.alloc((size_t)B * sizeof(float))); factor_cap = B; }
    if (r.keep_lat && evals > keep_tab_cap) { d_keep_tab = reinterpret_cast<float*>(pool.alloc((size_t)evals * 2 * sizeof(float))); keep_tab_cap = evals; }
    if (!ev[0]) for (auto& e : ev) HIP_OK(hipEventCreate(&e));
    // a table with a stochastic term (Euler-ancestral, DDIM with eta > 0, LCM, TCD with eta > 0): the caller's per-step noise is copied into
    // a runtime-owned buffer (upload_tables, on the run's stream) so that the pointer the captured graph holds stays valid after the caller
    // frees theirs.  One slab per evaluation, whichever rows read theirs (the last row of LCM and TCD has c_n = 0: its slab is never read)
    r.use_step_noise = table_needs_step_noise(r.table);
    r.step_noise_bytes = r.use_step_noise ? (size_t)evals * B * 4 * r.hw * sizeof(float) : 0;
    if (r.use_step_noise) {
        const int kind = decode_sched_code(r.in.scheduler).kind;
        const char* noisy = kind == SCHED_EULER_A ? "EulerAncestralDiscrete" : kind == SCHED_LCM ? "LCM" : kind == SCHED_TCD ? "TCD with eta > 0"
                                                                                                                         : "DDIM with eta > 0";
        if (!step_noise_src) { set_error(std::string("tryon: ") + noisy + " needs per-step noise (ladi_tryon_set_step_noise)"); return -7; }
        if (step_noise_steps < evals) {
            set_error(std::string("tryon: ") + noisy + " needs " + std::to_string(evals) + " steps of noise, ladi_tryon_set_step_noise gave " +
                      std::to_string(step_noise_steps));
            return -7;
        }
        if (r.step_noise_bytes > step_noise_cap) {
            if (step_noise_buf) HIP_OK(hipFree(step_noise_buf));
            step_noise_buf = nullptr; step_noise_cap = 0;
            HIP_OK(hipMalloc(reinterpret_cast<void**>(&step_noise_buf), r.step_noise_bytes));
            step_noise_cap = r.step_noise_bytes;
        }
    }
    if (ip_pos) {
        const size_t need = (size_t)r.n * (ip_T > 0 ? ip_T : 1) * unet->ip_E;
        if (need > ip_buf_cap) {
            if (ip_buf) HIP_OK_RC(hipFree(ip_buf));
            ip_buf = nullptr; ip_buf_cap = 0;
            HIP_OK_RC(hipMalloc(reinterpret_cast<void**>(&ip_buf), need * sizeof(h16)));
            ip_buf_cap = need;
        }
    }
    // every argument check is behind us: only now grow the feature cache (a refused run leaves it, and the graphs that hold it, alone)
    if (p.fc_on) {
        const size_t need = (size_t)r.n * r.hw * unet->fc_channels(fc_branch);
        if (need > fcache_cap) {
            if (fcache) HIP_OK_RC(hipFree(fcache));
            fcache = nullptr; fcache_cap = 0;
            HIP_OK_RC(hipMalloc(reinterpret_cast<void**>(&fcache), need * sizeof(h16)));
            fcache_cap = need;
        }
    }
    return 0;
}

void TryOn::upload_tables(Run& r) {
    const EvalPlan& p = r.plan;
    const int evals = r.evals;
    hipStream_t st = r.st;
    // attached range probes start the run from zero (here, never inside the replayed graph): UNet slots then accumulate
    // over all evaluations of this run
    Probe* pr[3] = {unet->probe, vae->probe, emasc ? emasc->probe : nullptr};
    for (int i = 0; i < 3; ++i)
        if (pr[i] && !(i > 0 && pr[i] == pr[0]) && !(i > 1 && pr[i] == pr[1])) pr[i]->reset(st);
    HIP_OK(hipMemcpyAsync(d_table, r.table.data(), (size_t)evals * sizeof(StepTable), hipMemcpyHostToDevice, st));
    HIP_OK(hipMemsetAsync(d_step, 0, 2 * sizeof(int), st));    // evaluation index + the step kernel's arrival ticket
    if (p.guided) HIP_OK(hipMemcpyAsync(d_gtab, p.gtab.data(), (size_t)evals * sizeof(float), hipMemcpyHostToDevice, st));
    if (p.pag_on) HIP_OK(hipMemcpyAsync(d_pag, pag_sched.data(), (size_t)evals * sizeof(float), hipMemcpyHostToDevice, st));
    if (r.keep_lat) HIP_OK(hipMemcpyAsync(d_keep_tab, r.keep_tab.data(), (size_t)evals * 2 * sizeof(float), hipMemcpyHostToDevice, st));
    if (p.sag_on) {
        HIP_OK(hipMemcpyAsync(d_sag_tab, r.sag_tab.data(), (size_t)evals * 4 * sizeof(float), hipMemcpyHostToDevice, st));
        HIP_OK(hipMemcpyAsync(d_sag, &sag_scale, sizeof(float), hipMemcpyHostToDevice, st));
    }
    if (r.use_step_noise) HIP_OK(hipMemcpyAsync(step_noise_buf, step_noise_src, r.step_noise_bytes, hipMemcpyDeviceToDevice, st));
    std::vector<float> tsf(r.timesteps.begin(), r.timesteps.end());
    if (unet->compute_temb(tsf.data(), evals, st)) { r.rc = -5; return; }
    HIP_OK(hipEventRecord(ev[0], st));
}

void TryOn::encode(Run& r) {
    const TryOnInputs& in = r.in;
    const EvalPlan& p = r.plan;
    Ctx& c = r.c;
    hipStream_t st = r.st;
    const int B = r.B, H = r.H, W = r.W, h = r.h, w = r.w, hw = r.hw, L = r.L, D = r.D, n = r.n, pose_ch = r.pose_ch;
    const bool has_cloth = r.has_cloth, keep_lat = r.keep_lat;
    // ---------------- persistent buffers for this call
    h16* ehs = r.ehs = c.alloc_h16((size_t)n * L * D);
    h16* mask_bin = r.mask_bin = c.alloc_h16((size_t)B * H * W);
    h16* mask2 = r.mask2 = c.alloc_h16((size_t)B * (H / 2) * (W / 2));
    h16* mask4 = r.mask4 = c.alloc_h16((size_t)B * (H / 4) * (W / 4));
    h16* mask8 = r.mask8 = c.alloc_h16((size_t)B * hw);
    h16* pose_lat = r.pose_lat = c.alloc_h16((size_t)B * hw * pose_ch);
    float* cloth_lat = r.cloth_lat = c.alloc_f32((size_t)B * hw * 4);
    float* masked_lat = r.masked_lat = c.alloc_f32((size_t)B * hw * 4);
    float* latents = r.latents = c.alloc_f32((size_t)B * hw * 4);
    r.cur_sample = c.alloc_f32((size_t)B * hw * 4);
    r.ets = c.alloc_f32((size_t)4 * B * hw * 4);
    Act& unet_in = r.unet_in = c.new_act(r.rows, h, w, 64);
    if (emasc) {
        const int sh[5] = {H, H, H / 2, H / 4, H / 8}, sw[5] = {W, W, W / 2, W / 4, W / 8};
        for (int i = 0; i < 5; ++i) r.skips[i] = c.new_act(B, sh[i], sw[i], emasc->cfg.out_ch[i]);
    }
    // preserve-unmasked latent blend: runtime-owned for the whole run (the captured graph holds these, never the caller's noise)
    float* keep_x0 = r.keep_x0 = keep_lat ? c.alloc_f32((size_t)B * hw * 4) : nullptr;
    float* keep_noise = r.keep_noise = keep_lat ? c.alloc_f32((size_t)B * hw * 4) : nullptr;
    float* keep_mask = r.keep_mask = keep_lat ? c.alloc_f32((size_t)B * hw) : nullptr;
    const size_t mk_persist = arena.mark();

    // the image context's shape is part of what the planning pass of the forward sees (which blocks take the chain of projections)
    if (!ip_pos) unet->clear_ip_context();
    else if (c.dry()) unet->ip_reserve(n, unet->ip_N);
    if (!c.dry()) {
        if (stats_cap) HIP_OK(hipMemsetAsync(stats, 0, stats_cap * sizeof(float), st));
        // prompt embeddings [uncond ; cond] (tryon_pipe.py:620-628)
        const size_t pe = (size_t)B * L * D * sizeof(h16);
        if (p.cfg) {
            HIP_OK(hipMemcpyAsync(ehs, in.negative_prompt_embeds, pe, hipMemcpyDeviceToDevice, st));
            HIP_OK(hipMemcpyAsync(ehs + (size_t)B * L * D, in.prompt_embeds, pe, hipMemcpyDeviceToDevice, st));
        } else HIP_OK(hipMemcpyAsync(ehs, in.prompt_embeds, pe, hipMemcpyDeviceToDevice, st));
        // PAG: [neg ; pe ; pe] -- the perturbed group has the cond group's context
        if (p.pag_on) HIP_OK(hipMemcpyAsync(ehs + (size_t)p.ng * B * L * D, in.prompt_embeds, pe, hipMemcpyDeviceToDevice, st));
        if (unet->set_context(ehs, n, L, st)) { r.rc = -6; return; }
        // image embeddings, the same groups: [neg ; pos], the perturbed group a copy of pos; a null negative is zeros
        if (ip_pos) {
            const size_t ie = (size_t)B * (ip_T > 0 ? ip_T : 1) * unet->ip_E;     // rows of E halves, or of T * E with a Plus adapter
            for (int g = 0; g < p.groups; ++g) {
                h16* dst = ip_buf + (size_t)g * ie;
                if (p.cfg && g == 0) {
                    if (ip_neg) HIP_OK(hipMemcpyAsync(dst, ip_neg, ie * sizeof(h16), hipMemcpyDeviceToDevice, st));
                    else HIP_OK(hipMemsetAsync(dst, 0, ie * sizeof(h16), st));
                } else HIP_OK(hipMemcpyAsync(dst, ip_pos, ie * sizeof(h16), hipMemcpyDeviceToDevice, st));
            }
            if (ip_T > 0 ? unet->set_ip_context_seq(ip_buf, n, ip_T, st) : unet->set_ip_context(ip_buf, n, st)) { r.rc = -6; return; }
        }
    }
    // ---------------- 4. mask / masked image / pose (tryon_pipe.py:630-636)
    Act masked_img = c.new_act(B, H, W, 64);
    if (!c.dry()) {
        c.check(ladi_launch_prepare_mask(in.image, in.in_f32, in.mask_image, in.in_f32, B, H, W, masked_img.p, 64, mask_bin, st), "prepare_mask");
        c.check(ladi_launch_mask_down(mask_bin, B, H, W, 2, mask2, st), "mask_down");
        c.check(ladi_launch_mask_down(mask_bin, B, H, W, 4, mask4, st), "mask_down");
        c.check(ladi_launch_mask_down(mask_bin, B, H, W, 8, mask8, st), "mask_down");
        if (in.no_pose) HIP_OK(hipMemsetAsync(pose_lat, 0, (size_t)B * hw * pose_ch * sizeof(h16), st));
        else c.check(ladi_launch_pose_down8(in.pose_map, in.in_f32, B, pose_ch, H, W, pose_lat, st), "pose_down8");
    }
    // ---------------- 4b. cloth latents (RNG draw #1)
    if (has_cloth) {
        const size_t mk = arena.mark();
        Act cloth = c.new_act(B, H, W, 64);
        if (!c.dry()) c.check(ladi_launch_nchw_to_nhwc(in.warped_cloth, in.in_f32, B, 3, H, W, cloth.p, 64, st), "nchw_to_nhwc");
        Act feats[5];
        c.stats_off = 0;
        Act mom = vae->encode(c, cloth, feats);
        if (!c.dry()) c.check(ladi_launch_posterior_sample(mom.p, mom.ld, in.noise_cloth, B, hw, vae->cfg.scaling_factor, cloth_lat, st), "posterior");
        arena.release(mk);
    }
    // ---------------- 4c. preserve-unmasked: z0 = scaling * mode(encode(image)) (no RNG draw), the noise, the keep mask
    if (keep_lat) {
        const size_t mk = arena.mark();
        Act full = c.new_act(B, H, W, 64);
        if (!c.dry()) {
            c.check(ladi_launch_nchw_to_nhwc(in.image, in.in_f32, B, 3, H, W, full.p, 64, st), "nchw_to_nhwc");
            if (stats_cap) HIP_OK(hipMemsetAsync(stats, 0, stats_cap * sizeof(float), st));
        }
        Act feats[5];
        c.stats_off = 0;
        Act mom = vae->encode(c, full, feats);
        if (!c.dry()) {
            c.check(ladi_launch_posterior_sample(mom.p, mom.ld, nullptr, B, hw, vae->cfg.scaling_factor, keep_x0, st), "posterior mode");
            c.check(ladi_launch_lat_nchw_to_pix(in.noise_latents, B, hw, 1.f, keep_noise, st), "keep noise");
            c.check(ladi_launch_mask_pool8(mask_bin, B, H, W, 1, keep_mask, st), "mask_pool8");
        }
        arena.release(mk);
    }
    // ---------------- 6. initial latents (RNG draw #2) * init_noise_sigma (1 for DDIM / PNDM; tryon_pipe.py:424)
    // with an init (strength): k_x * resample(init) + k_n * noise, or the init itself (init_noisy); init_noise_sigma is not applied
    if (!c.dry() && r.first_step)
        c.check(ladi_launch_init_latents(init_src, init_hs, init_ws, init_noisy ? nullptr : in.noise_latents, B, h, w,
                                         init_noisy ? 1.f : r.sinfo.start_kx, init_noisy ? 0.f : r.sinfo.start_kn, latents, st), "init_latents");
    else if (!c.dry()) c.check(ladi_launch_lat_nchw_to_pix(in.noise_latents, B, hw, r.sinfo.init_noise_sigma, latents, st), "latents");
    // ---------------- 7. masked-image latents (RNG draw #3) + EMASC skips
    {
        Act feats[5];
        if (!c.dry()) if (stats_cap) HIP_OK(hipMemsetAsync(stats, 0, stats_cap * sizeof(float), st));
        c.stats_off = 0;
        Act mom = vae->encode(c, masked_img, feats);
        if (!c.dry()) c.check(ladi_launch_posterior_sample(mom.p, mom.ld, in.noise_masked, B, hw, vae->cfg.scaling_factor, masked_lat, st), "posterior");
        if (emasc) {
            const h16* masks[5] = {mask_bin, mask_bin, mask2, mask4, mask8};
            emasc->forward(c, feats, masks, r.skips, true);
        }
    }
    arena.release(mk_persist);
    // ---------------- 7a. static UNet input channels
    if (!c.dry()) {
        const bool cloth_zero_from_start = has_cloth && in.cloth_zero_from <= 0;
        c.check(ladi_launch_assemble_static(unet_in.p, 64, B, hw, p.cfg ? 1 : 0, latents, mask8, masked_lat, pose_lat, pose_ch,
                                            (has_cloth && !cloth_zero_from_start) ? cloth_lat : nullptr, has_cloth ? 1 : 0,
                                            r.sinfo.in_scale0, st, p.pag_on ? 1 : 0), "assemble");
        HIP_OK(hipEventRecord(ev[1], st));
    }
}

// ---------------- 9. denoising loop
void TryOn::denoise(Run& r) {
    const TryOnInputs& in = r.in;
    const EvalPlan& p = r.plan;
    Ctx& c = r.c;
    hipStream_t st = r.st;
    const int B = r.B, hw = r.hw, evals = r.evals, cfgf = p.cfg ? 1 : 0;
    const Act& unet_in = r.unet_in;
    float* latents = r.latents;
    StepArgs sa; std::memset(&sa, 0, sizeof(sa));
    sa.B = B; sa.hw = hw; sa.cfg = cfgf; sa.guidance = in.guidance; sa.latents = latents; sa.cur_sample = r.cur_sample; sa.ets = r.ets;
    sa.table = d_table; sa.step_idx = d_step; sa.unet_in = unet_in.p; sa.ld_in = 64; sa.cloth_ch0 = 9 + r.pose_ch;
    sa.trace_eps = trace_eps; sa.trace_lat = trace_lat; sa.trace_cap = trace_cap;
    sa.step_noise = r.use_step_noise ? step_noise_buf : nullptr;
    sa.guidance_tab = p.guided ? d_gtab : nullptr;
    sa.factor = p.use_factor ? d_factor : nullptr;
    sa.pag_tab = p.pag_on ? d_pag : nullptr;
    sa.sag_scale = p.sag_on ? d_sag : nullptr;
    int sag_hm = 0, sag_wm = 0;
    UNet::sag_tokens(r.h, r.w, &sag_hm, &sag_wm);
    if (r.keep_lat) { sa.keep_x0 = r.keep_x0; sa.keep_noise = r.keep_noise; sa.keep_mask = r.keep_mask; sa.keep_tab = d_keep_tab; }
    // the UNet forward runs as lanes.G independent sample groups on as many streams (runtime.h UNetLanes); the lanes own their
    // arenas, the shared noise prediction lives in this one
    const int eps_ld = (unet->cfg.out_channels + 3) / 4 * 4;
    Act eps = c.new_act(r.rows, r.h, r.w, unet->cfg.out_channels, eps_ld);
    const size_t mk_loop = arena.mark();
    // one evaluation of form f (runtime.h GraphTable).  Bit 0, cond-only evaluation of a guided run: the UNet runs over the conditional
    // samples [B, 2B) (their rows of unet_in and eps, their part of the K/V cache) and the step kernel, told by the table, reads only those
    // rows of eps.  Bit 1, shallow evaluation (feature cache); a whole evaluation of a cached run captures.  Bit 2, PAG evaluation: the
    // forward also runs over the perturbed group, the rows behind the cond group's, perturbed from sample ng * B of the context batch; in a
    // PAG-shaped run an evaluation without PAG runs over the rows [0, ng * B) or [B, 2B).  All rows from sample 0 are the whole-batch call
    auto one_step = [&](bool concurrent, int f) {
        const bool cond = f & 1, sh = f & 2, pg = f & 4;
        arena.release(mk_loop);
        FeatCache fcs; fcs.mode = sh ? FeatCache::SHALLOW : FeatCache::CAPTURE; fcs.branch = fc_branch; fcs.buf = fcache;
        const int s0 = cond ? B : 0, ns = ((cond ? 1 : p.ng) + (pg ? 1 : 0)) * B;
        Act xs = unet_in, es = eps;
        xs.n = ns; xs.p = unet_in.p + (size_t)s0 * hw * unet_in.ld;
        es.n = ns; es.p = eps.p + (size_t)s0 * hw * eps.ld;
        FwdOpt fo; fo.sample0 = s0; fo.fc = p.fc_on ? &fcs : nullptr; fo.pag_first = pg ? p.ng * B : (int)PAG_NONE;
        if (p.sag_on) fo.sag = 1;
        lanes.forward(*unet, st, c.dry(), concurrent, xs, es, unet->temb_table, d_step, fo);
        // SAG: degrade the latents where the base group (the first group of this evaluation: uncond under CFG, else cond) attends most, into
        // the rows behind the last group, and run those B samples with the base group's context rows; the map stays the first forward's
        if (p.sag_on) {
            const size_t d0 = (size_t)p.ng * B;
            Act xd = unet_in, ed = eps;
            xd.n = B; xd.p = unet_in.p + d0 * hw * unet_in.ld;
            ed.n = B; ed.p = eps.p + d0 * hw * eps.ld;
            if (!c.dry())
                c.check(ladi_launch_sag_degrade(latents, es.p, eps.ld, unet->sag_m + (size_t)s0 * unet->sag_T, B, r.h, r.w, sag_hm, sag_wm, d_sag_tab,
                                                d_step, xs.p, xd.p, unet_in.ld, unet_in.ld, st), "sag_degrade");
            FwdOpt f2; f2.sample0 = s0; f2.sag = 0;
            lanes.forward(*unet, st, c.dry(), concurrent, xd, ed, unet->temb_table, d_step, f2);
        }
        if (c.dry()) return;
        sa.eps = eps.p; sa.ld_eps = eps.ld;
        if (p.use_factor && !cond)
            c.check(p.sag_on ? ladi_launch_cfg_stats_sag(eps.p, eps.ld, B, hw, d_gtab, d_step, 0.f, d_sag, 0.f, phi, d_factor, st)
                    : p.pag_on ? ladi_launch_cfg_stats_pag(eps.p, eps.ld, B, hw, d_gtab, d_step, 0.f, d_pag, 0.f, phi, d_factor, st)
                               : ladi_launch_cfg_stats(eps.p, eps.ld, B, hw, d_gtab, d_step, 0.f, phi, d_factor, st), "cfg_stats");
        c.check(ladi_launch_sched_step(sa, st), "sched_step");
    };
    // step callback after evaluation i (between launches, never inside a capture): latents out to the caller's NCHW buffer, the host
    // call, the buffer back into the loop and the next UNet input.  Work the callback queued on the caller's stream comes first.
    // A non-zero return of the callback lands in cb_rc and ends the loop (the run is then aborted).  No callback set: nothing is
    // launched and nothing waits.
    auto callback_point = [&](int i) {
        if (!cb_fn || i % cb_every) return;
        c.check(ladi_launch_lat_pix_to_nchw(latents, B, hw, cb_latents, st), "callback export");
        HIP_OK(hipStreamSynchronize(st));
        r.cb_eval = i;
        if ((r.cb_rc = cb_fn(cb_user, i)) != 0) return;
        HIP_OK(hipEventRecord(ev_in, r.user_st));
        HIP_OK(hipStreamWaitEvent(st, ev_in, 0));
        c.check(ladi_launch_latents_import(cb_latents, B, hw, latents, unet_in.p, 64, cfgf, r.table[i].in_scale_next, st, p.pag_on ? 1 : 0),
                "callback import");
    };
    // the first evaluation of any form runs its lanes one after the other (one-time function attribute setup, per-shape tile measurement)
    bool seen[GraphTable::N] = {};
    // an evaluation whose forward ran over B samples (launched eagerly or by replaying the cond-only graph; every one of a run without CFG)
    auto ran = [&](int f) { if ((f & 1) || !cfgf) ++last_cond_only; if (f & 2) ++last_shallow; };
    if (c.dry()) {
        // the planning pass: the whole evaluation and every form this run has
        for (int f = 0; f < GraphTable::N; ++f) if (f == 0 || p.has_form[f]) one_step(false, f);
    } else if (!in.use_graph || evals < 3) {
        for (int i = 0; i < evals && !r.cb_rc; ++i) {
            const int f = p.form[i];
            one_step(i > 0 && seen[f], f); seen[f] = true; ran(f);
            callback_point(i);
        }
    } else {
        one_step(false, p.form[0]);  // eager first evaluation (always whole)
        seen[p.form[0]] = true; ran(p.form[0]);
        callback_point(0);
        GraphKey key; std::memset(&key, 0, sizeof(key));
        key.arena = arena.base; key.B = B; key.H = r.H; key.W = r.W; key.cfg = cfgf; key.L = r.L; key.pose_ch = r.pose_ch; key.has_cloth = r.has_cloth;
        if (!p.guided) std::memcpy(&key.guidance, &in.guidance, 4);
        key.d_table = d_table; key.stats = stats;
        key.trace_eps = trace_eps; key.trace_lat = trace_lat; key.trace_cap = trace_cap;
        key.step_noise = sa.step_noise;
        lanes.key(key.lanes);
        unet->key(key.unet, p.pag_on, p.sag_on ? 1 : -1);
        if (p.sag_on) { key.sag_on = 1; key.sag_scale = d_sag; key.sag_tab = d_sag_tab; }
        key.guidance_tab = sa.guidance_tab; key.factor = sa.factor; key.guided = p.guided;
        if (p.guided) std::memcpy(&key.phi, &phi, 4);
        if (p.fc_on) { key.fcache = fcache; key.fc_on = 1; key.fc_branch = fc_branch; }
        key.keep_x0 = sa.keep_x0; key.keep_noise = sa.keep_noise; key.keep_mask = sa.keep_mask; key.keep_tab = sa.keep_tab;
        if (r.keep_lat) key.preserve_mode = preserve_mode;
        key.pag_on = p.pag_on ? 1 : 0; key.pag_tab = sa.pag_tab;
        if (std::memcmp(&key, &graph_key, sizeof(key))) { graphs.clear(); std::memcpy(&graph_key, &key, sizeof(key)); }
        // the host knows the schedule and picks the graph; the values come from the device table.  A form that this run has not yet
        // run eagerly and that has no graph runs eagerly once (see above), its next evaluation captures
        for (int i = 1; i < evals && !r.cb_rc; ++i) {
            const int f = p.form[i];
            if (!graphs.e[f] && !seen[f]) { one_step(false, f); seen[f] = true; }
            else {
                if (!graphs.e[f]) graphs.capture(f, st, [&]() { one_step(true, f); });
                HIP_OK(hipGraphLaunch(graphs.e[f], st));
            }
            ran(f);
            callback_point(i);
        }
    }
    arena.release(mk_loop);
    if (!c.dry() && !r.cb_rc) HIP_OK(hipEventRecord(ev[2], st));
}

// ---------------- 11. decode (tryon_pipe.py:349-359)
void TryOn::decode(Run& r) {
    Ctx& c = r.c;
    hipStream_t st = r.st;
    const int B = r.B, H = r.H, W = r.W, hw = r.hw;
    float* latents = r.latents;
    const Act* skips = emasc ? r.skips : nullptr;
    Act z = c.new_act(B, r.h, r.w, 64);
    // pixel composite with a feathered mask: the blurred mask and the row pass's scratch
    const bool feather = r.keep_pix && preserve_sigma > 0.f;
    float* m_soft = feather ? c.alloc_f32((size_t)B * H * W) : nullptr;
    float* m_tmp = feather ? c.alloc_f32((size_t)B * H * W) : nullptr;
    if (!c.dry()) {
        if (stats_cap) HIP_OK(hipMemsetAsync(stats, 0, stats_cap * sizeof(float), st));
        c.check(ladi_launch_post_quant(latents, vae->d_pq, 1.0f / vae->cfg.scaling_factor, B * hw, z.p, 64, st), "post_quant");
    }
    // decode under the fp16-range guard (runtime.h VAE::range_shift): the planning pass reserves the guarded form's arena (a
    // superset: scaled copies of the skips); the real pass re-runs the decode with more head-room only if a GroupNorm of the
    // decoder saw non-finite statistics
    const size_t mk_dec = arena.mark();
    if (c.dry()) {
        c.stats_off = 0;
        (void)vae->decode(c, z, skips, vae->range_shift < 0 ? 4 : vae->range_shift);
        return;
    }
    // ONE decode at the guard's current shift; the flag is examined without a host round trip (runtime.h VAE::post_overflow_check /
    // poll_overflow: at the entry of the next run, or by ladi_tryon_poll_overflow)
    const int sh = vae->guard_shift();
    arena.release(mk_dec);
    c.stats_off = 0;
    if (stats_cap) HIP_OK(hipMemsetAsync(stats, 0, stats_cap * sizeof(float), st));
    Act img = vae->decode(c, z, skips, sh);
    if (r.keep_pix) {
        if (feather) c.check(ladi_launch_mask_feather(r.mask_bin, B, H, W, preserve_sigma, m_tmp, m_soft, st), "mask_feather");
        c.check(ladi_launch_image_composite(img.p, img.ld, r.in.image, r.in.in_f32, feather ? (const void*)m_soft : (const void*)r.mask_bin,
                                            feather ? 1 : 0, B, H * W, r.images_out, r.images_u8, st), "image_composite");
    } else c.check(ladi_launch_image_post(img.p, img.ld, B * H * W, r.images_out, r.images_u8, st), "image_post");
    vae->last_shift = sh;
    vae->post_overflow_check(st);
    if (r.latents_out) c.check(ladi_launch_lat_pix_to_nchw(latents, B, hw, r.latents_out, st), "latents_out");
    HIP_OK(hipEventRecord(ev[3], st));
    ev_valid = true;
}

}  // namespace ladi
