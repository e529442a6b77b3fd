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

TryOn::~TryOn() {
    if (gexec) (void)hipGraphExecDestroy(gexec);
    if (graph) (void)hipGraphDestroy(graph);
    if (gexec_cond) (void)hipGraphExecDestroy(gexec_cond);
    if (graph_cond) (void)hipGraphDestroy(graph_cond);
    for (auto& g : gexec_sh) if (g) (void)hipGraphExecDestroy(g);
    for (auto& g : graph_sh) if (g) (void)hipGraphDestroy(g);
    for (auto& g : gexec_pag) if (g) (void)hipGraphExecDestroy(g);
    for (auto& g : graph_pag) if (g) (void)hipGraphDestroy(g);
    if (fcache) (void)hipFree(fcache);
    if (stats) (void)hipFree(stats);
    if (step_noise_buf) (void)hipFree(step_noise_buf);
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

static unsigned long long mix(unsigned long long h, unsigned long long v) {
    h ^= v + 0x9e3779b97f4a7c15ULL + (h << 6) + (h >> 2);
    return h;
}

int TryOn::run(const TryOnInputs& in, void* images_out, int images_u8, float* latents_out, hipStream_t user_st) {
    if (!unet || !vae) { set_error("tryon: unet and vae are required"); return -1; }
    hipStream_t st = user_st;
    try {
        if (!own_stream) {
            HIP_OK(hipStreamCreateWithFlags(&own_stream, hipStreamNonBlocking));
            HIP_OK(hipEventCreateWithFlags(&ev_in, hipEventDisableTiming));
            HIP_OK(hipEventCreateWithFlags(&ev_out, hipEventDisableTiming));
        }
        HIP_OK(hipEventRecord(ev_in, user_st));
        HIP_OK(hipStreamWaitEvent(own_stream, ev_in, 0));
        st = own_stream;
    } catch (const std::exception& e) { set_error(std::string("tryon: ") + e.what()); return -100; }
    try {
        if (vae->poll_overflow()) {      // the PREVIOUS run's decode left the fp16 range: its images are invalid and nobody asked (ladi_tryon_poll_overflow)
            set_error("tryon: the previous run's VAE decode overflowed the fp16 range (non-finite GroupNorm statistics) at range shift " + std::to_string(vae->last_shift) +
                      "; its images are invalid -- re-submit that batch (the automatic shift is now " + std::to_string(vae->guard_shift()) + ")");
            (void)hipEventRecord(ev_out, st); (void)hipStreamWaitEvent(user_st, ev_out, 0);
            return -101;
        }
    } catch (const std::exception& e) { set_error(std::string("tryon: ") + e.what()); return -100; }
    const int B = in.batch, H = in.height, W = in.width;
    if (H % 8 || W % 8) { set_error("height and width must be divisible by 8"); return -2; }
    const int h = H / 8, w = W / 8, hw = h * w;
    // per-evaluation guidance: the run is CFG-shaped if ANY evaluation's scale is > 1; a set schedule replaces in.guidance
    const bool has_sched = !g_sched.empty();
    bool any_cfg = in.guidance > 1.0f;
    if (has_sched) { any_cfg = false; for (float g : g_sched) any_cfg = any_cfg || g > 1.0f; }
    const int cfgf = any_cfg ? 1 : 0;
    // guided: the scales come from a device table (a schedule, or the scalar repeated for the rescale statistics); else today's scalar path
    const bool guided = cfgf && (has_sched || phi > 0.f);
    const int ng = cfgf ? 2 : 1;       // sample groups of a plain evaluation: [uncond ; cond] or [cond]
    const bool has_cloth = in.warped_cloth != nullptr;
    const int pose_ch = in.pose_channels;
    const int in_ch = 9 + pose_ch + (has_cloth ? 4 : 0);
    if (in_ch != unet->cfg.in_channels) { set_error("tryon: UNet in_channels does not match 9 + pose + cloth channels"); return -3; }
    const int L = in.L, D = unet->cfg.cross_dim;
    if (cfgf && !in.negative_prompt_embeds) { set_error("tryon: negative_prompt_embeds required when guidance_scale > 1"); return -4; }

    // ---- scheduler tables (host)
    std::vector<float> ac;
    if (in.alphas_cumprod) ac.assign(in.alphas_cumprod, in.alphas_cumprod + 1000); else default_alphas_cumprod(ac);
    std::vector<double> timesteps; std::vector<StepTable> table; SchedInfo sinfo;
    // a set init (ladi_tryon_set_init) starts the run at step first_step of the schedule: the tables below are the tail's, indexed from 0
    const int first_step = (init_src && init_first > 0) ? init_first : 0;
    build_step_table(in.scheduler, in.steps, ac.data(), in.cloth_zero_from, timesteps, table, &sinfo, eta, first_step);
    const int evals = (int)timesteps.size();
    if (has_sched && (int)g_sched.size() != evals) {
        set_error("tryon: the guidance schedule has " + std::to_string(g_sched.size()) + " entries, this run has " + std::to_string(evals) +
                  " evaluations (PNDM: steps + 1" + (first_step ? "; the run starts at step " + std::to_string(first_step) + " of " +
                  std::to_string(in.steps) : std::string()) + ")");
        return -9;
    }
    // perturbed-attention guidance: one scale per evaluation; the run is PAG-shaped (a third sample group) if ANY scale is > 0
    if (!pag_sched.empty() && (int)pag_sched.size() != evals) {
        set_error("tryon: the PAG table has " + std::to_string(pag_sched.size()) + " entries, this run has " + std::to_string(evals) +
                  " evaluations (PNDM: steps + 1" + (first_step ? "; the run starts at step " + std::to_string(first_step) + " of " +
                  std::to_string(in.steps) : std::string()) + ")");
        return -9;
    }
    bool pag_on = false;
    for (float s : pag_sched) pag_on = pag_on || s > 0.f;
    if (pag_on && !fc_plan.empty()) {
        set_error("tryon: perturbed-attention guidance together with a feature-cache plan is not supported (the cache's group promotion has "
                  "no third group): clear one of ladi_tryon_set_pag / ladi_tryon_set_feature_cache");
        return TRYON_PAG_WITH_CACHE;
    }
    auto pag_eval = [&](int i) { return pag_on && pag_sched[i] > 0.f; };
    const int n = (ng + (pag_on ? 1 : 0)) * B;
    // scale of evaluation i, and whether it runs cond-only (scale <= 1: no unconditional half, as do_classifier_free_guidance of a whole run)
    std::vector<float> gtab(evals, in.guidance);
    if (has_sched) gtab = g_sched;
    auto cond_only = [&](int i) { return guided && !(gtab[i] > 1.0f); };
    bool any_cond_only = false;
    for (int i = 0; i < evals; ++i) any_cond_only = any_cond_only || cond_only(i);
    // deep-feature cache plan (ladi_tryon_set_feature_cache): one flag per evaluation, 1 = whole forward.  A plan without a shallow evaluation
    // is the plain run: capture stays off.  The one promotion, on the host: a shallow evaluation over all 2B samples needs a cache whose two
    // halves were written by the same whole evaluation, so after a whole evaluation that ran cond-only (rows [B, 2B) only) it runs whole
    if (!fc_plan.empty()) {
        if ((int)fc_plan.size() != evals) {
            set_error("tryon: the feature-cache plan has " + std::to_string(fc_plan.size()) + " entries, this run has " + std::to_string(evals) +
                      " evaluations (PNDM: steps + 1" + (first_step ? "; the run starts at step " + std::to_string(first_step) + " of " +
                      std::to_string(in.steps) : std::string()) + ")");
            return -10;
        }
        if (!fc_plan[0]) { set_error("tryon: the feature-cache plan must start with a whole evaluation (flag 0 = 1)"); return -10; }
    }
    std::vector<unsigned char> whole(evals, 1);
    bool fc_on = false;
    if (!fc_plan.empty()) {
        bool halves_differ = false;      // the most recent whole evaluation refreshed the conditional rows only
        for (int i = 0; i < evals; ++i) {
            whole[i] = fc_plan[i] ? 1 : 0;
            if (!whole[i] && cfgf && !cond_only(i) && halves_differ) whole[i] = 1;
            if (whole[i]) halves_differ = cfgf && cond_only(i);
            fc_on = fc_on || !whole[i];
        }
    }
    last_shallow = 0;
    const bool use_factor = guided && phi > 0.f;
    const bool cloth_zero_from_start = has_cloth && in.cloth_zero_from <= 0;
    last_evals = evals;
    last_cond_only = 0;      // counted below, where an evaluation over B samples is actually launched

    if (!d_step) d_step = reinterpret_cast<int*>(pool.alloc(256));
    if (!sk_cnt) { sk_cnt = reinterpret_cast<int*>(pool.alloc(1024 * sizeof(int))); HIP_OK(hipMemset(sk_cnt, 0, 1024 * sizeof(int))); }
    if (evals > table_cap) { d_table = reinterpret_cast<StepTable*>(pool.alloc((size_t)evals * sizeof(StepTable))); table_cap = evals; }
    if (guided && evals > gtab_cap) { d_gtab = reinterpret_cast<float*>(pool.alloc((size_t)evals * sizeof(float))); gtab_cap = evals; }
    if (pag_on && evals > pag_cap) { d_pag = reinterpret_cast<float*>(pool.alloc((size_t)evals * sizeof(float))); pag_cap = evals; }
    if (use_factor && B > factor_cap) { d_factor = reinterpret_cast<float*>(pool.alloc((size_t)B * sizeof(float))); factor_cap = B; }
    // preserve-unmasked: the blend's coefficients per evaluation, float64 on the host like the step table
    const bool keep_lat = (preserve_mode & 1) != 0, keep_pix = (preserve_mode & 2) != 0;
    std::vector<float> keep_tab;
    if (keep_lat) {
        keep_coeffs_of(in.scheduler, timesteps, sinfo, ac.data(), first_step, keep_tab);
        if (evals > keep_tab_cap) { d_keep_tab = reinterpret_cast<float*>(pool.alloc((size_t)evals * 2 * sizeof(float))); keep_tab_cap = evals; }
    }
    if (!ev[0]) for (auto& e : ev) HIP_OK(hipEventCreate(&e));
    // a table with a stochastic term (Euler-ancestral, DDIM with eta > 0): the caller's per-step noise is copied into a runtime-owned buffer
    // (below, on the run's stream) so that the pointer the captured graph holds stays valid after the caller frees theirs
    const bool use_step_noise = table_needs_step_noise(table);
    const size_t step_noise_bytes = use_step_noise ? (size_t)evals * B * 4 * hw * sizeof(float) : 0;
    const char* noisy = decode_sched_code(in.scheduler).kind == SCHED_EULER_A ? "EulerAncestralDiscrete" : "DDIM with eta > 0";
    if (use_step_noise) {
        if (!step_noise_src) { set_error(std::string("tryon: ") + noisy + " needs per-step noise (ladi_tryon_set_step_noise)"); return -7; }
        if (step_noise_steps < evals) {
            set_error(std::string("tryon: ") + noisy + " needs " + std::to_string(evals) + " steps of noise, ladi_tryon_set_step_noise gave " +
                      std::to_string(step_noise_steps));
            return -7;
        }
        if (step_noise_bytes > step_noise_cap) {
            if (step_noise_buf) HIP_OK(hipFree(step_noise_buf));
            step_noise_buf = nullptr; step_noise_cap = 0;
            HIP_OK(hipMalloc(reinterpret_cast<void**>(&step_noise_buf), step_noise_bytes));
            step_noise_cap = step_noise_bytes;
        }
    }
    // every argument check is behind us: only now grow the feature cache (a refused run leaves it, and the graphs that hold it, alone)
    if (fc_on) {
        const size_t need = (size_t)n * hw * unet->fc_channels(fc_branch);
        if (need > fcache_cap) {
            if (fcache) HIP_OK_RC(hipFree(fcache));
            fcache = nullptr; fcache_cap = 0;
            HIP_OK_RC(hipMalloc(reinterpret_cast<void**>(&fcache), need * sizeof(h16)));
            fcache_cap = need;
        }
    }

    int rc = 0;      // -5 / -6: time embedding / context failed in the real pass (the error is set; the streams are joined like on success)
    try {
        lanes.configure(n, lanes_override > 0 && (n % lanes_override) == 0 ? lanes_override : 0);
        for (int pass = 0; pass < 2; ++pass) {
            arena.dry = (pass == 0);
            arena.off = 0;
            Ctx c; c.st = st; c.ar = &arena; c.stats = stats; c.stats_cap = stats_cap; c.sk_cnt = sk_cnt;
            if (pass == 1) {
                // attached range probes start the run from zero (here, never inside the replayed graph): UNet slots then accumulate
                // over all evaluations of this run
                Probe* pr[3] = {unet->probe, vae->probe, emasc ? emasc->probe : nullptr};
                for (int i = 0; i < 3; ++i)
                    if (pr[i] && !(i > 0 && pr[i] == pr[0]) && !(i > 1 && pr[i] == pr[1])) pr[i]->reset(st);
                HIP_OK(hipMemcpyAsync(d_table, table.data(), (size_t)evals * sizeof(StepTable), hipMemcpyHostToDevice, st));
                HIP_OK(hipMemsetAsync(d_step, 0, 2 * sizeof(int), st));    // evaluation index + the step kernel's arrival ticket
                if (guided) HIP_OK(hipMemcpyAsync(d_gtab, gtab.data(), (size_t)evals * sizeof(float), hipMemcpyHostToDevice, st));
                if (pag_on) HIP_OK(hipMemcpyAsync(d_pag, pag_sched.data(), (size_t)evals * sizeof(float), hipMemcpyHostToDevice, st));
                if (keep_lat) HIP_OK(hipMemcpyAsync(d_keep_tab, keep_tab.data(), (size_t)evals * 2 * sizeof(float), hipMemcpyHostToDevice, st));
                if (use_step_noise) HIP_OK(hipMemcpyAsync(step_noise_buf, step_noise_src, step_noise_bytes, hipMemcpyDeviceToDevice, st));
                std::vector<float> tsf(timesteps.begin(), timesteps.end());
                if (unet->compute_temb(tsf.data(), evals, st)) { rc = -5; break; }
                HIP_OK(hipEventRecord(ev[0], st));
            }
            // ---------------- persistent buffers for this call
            h16* ehs = c.alloc_h16((size_t)n * L * D);
            h16* mask_bin = c.alloc_h16((size_t)B * H * W);
            h16* mask2 = c.alloc_h16((size_t)B * (H / 2) * (W / 2));
            h16* mask4 = c.alloc_h16((size_t)B * (H / 4) * (W / 4));
            h16* mask8 = c.alloc_h16((size_t)B * hw);
            h16* pose_lat = c.alloc_h16((size_t)B * hw * pose_ch);
            float* cloth_lat = c.alloc_f32((size_t)B * hw * 4);
            float* masked_lat = c.alloc_f32((size_t)B * hw * 4);
            float* latents = c.alloc_f32((size_t)B * hw * 4);
            float* cur_sample = c.alloc_f32((size_t)B * hw * 4);
            float* ets = c.alloc_f32((size_t)4 * B * hw * 4);
            Act unet_in = c.new_act(n, h, w, 64);
            Act skips[5];
            const bool use_emasc = emasc != nullptr;
            if (use_emasc) {
                const int sh[5] = {H, H, H / 2, H / 4, H / 8}, sw[5] = {W, W, W / 2, W / 4, W / 8};
                for (int i = 0; i < 5; ++i) skips[i] = c.new_act(B, sh[i], sw[i], emasc->cfg.out_ch[i]);
            }
            // preserve-unmasked latent blend: runtime-owned for the whole run (the captured graph holds these, never the caller's noise)
            float* keep_x0 = keep_lat ? c.alloc_f32((size_t)B * hw * 4) : nullptr;
            float* keep_noise = keep_lat ? c.alloc_f32((size_t)B * hw * 4) : nullptr;
            float* keep_mask = keep_lat ? c.alloc_f32((size_t)B * hw) : nullptr;
            const size_t mk_persist = arena.mark();

            if (!c.dry()) {
                if (stats_cap) HIP_OK(hipMemsetAsync(stats, 0, stats_cap * sizeof(float), st));
                // prompt embeddings [uncond ; cond] (tryon_pipe.py:620-628)
                const size_t pe = (size_t)B * L * D * sizeof(h16);
                if (cfgf) {
                    HIP_OK(hipMemcpyAsync(ehs, in.negative_prompt_embeds, pe, hipMemcpyDeviceToDevice, st));
                    HIP_OK(hipMemcpyAsync(ehs + (size_t)B * L * D, in.prompt_embeds, pe, hipMemcpyDeviceToDevice, st));
                } else HIP_OK(hipMemcpyAsync(ehs, in.prompt_embeds, pe, hipMemcpyDeviceToDevice, st));
                // PAG: [neg ; pe ; pe] -- the perturbed group has the cond group's context
                if (pag_on) HIP_OK(hipMemcpyAsync(ehs + (size_t)ng * B * L * D, in.prompt_embeds, pe, hipMemcpyDeviceToDevice, st));
                if (unet->set_context(ehs, n, L, st)) { rc = -6; break; }
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
            if (!c.dry() && first_step)
                c.check(ladi_launch_init_latents(init_src, init_hs, init_ws, init_noisy ? nullptr : in.noise_latents, B, h, w,
                                                 init_noisy ? 1.f : sinfo.start_kx, init_noisy ? 0.f : sinfo.start_kn, latents, st), "init_latents");
            else if (!c.dry()) c.check(ladi_launch_lat_nchw_to_pix(in.noise_latents, B, hw, sinfo.init_noise_sigma, latents, st), "latents");
            // ---------------- 7. masked-image latents (RNG draw #3) + EMASC skips
            {
                Act feats[5];
                if (!c.dry()) if (stats_cap) HIP_OK(hipMemsetAsync(stats, 0, stats_cap * sizeof(float), st));
                c.stats_off = 0;
                Act mom = vae->encode(c, masked_img, feats);
                if (!c.dry()) c.check(ladi_launch_posterior_sample(mom.p, mom.ld, in.noise_masked, B, hw, vae->cfg.scaling_factor, masked_lat, st), "posterior");
                if (use_emasc) {
                    const h16* masks[5] = {mask_bin, mask_bin, mask2, mask4, mask8};
                    emasc->forward(c, feats, masks, skips, true);
                }
            }
            arena.release(mk_persist);
            // ---------------- 7a. static UNet input channels
            if (!c.dry()) {
                c.check(ladi_launch_assemble_static(unet_in.p, 64, B, hw, cfgf, latents, mask8, masked_lat, pose_lat, pose_ch,
                                                    (has_cloth && !cloth_zero_from_start) ? cloth_lat : nullptr, has_cloth ? 1 : 0,
                                                    sinfo.in_scale0, st, pag_on ? 1 : 0), "assemble");
                HIP_OK(hipEventRecord(ev[1], st));
            }
            // ---------------- 9. denoising loop
            StepArgs sa; std::memset(&sa, 0, sizeof(sa));
            sa.B = B; sa.hw = hw; sa.cfg = cfgf; sa.guidance = in.guidance; sa.latents = latents; sa.cur_sample = cur_sample; sa.ets = ets;
            sa.table = d_table; sa.step_idx = d_step; sa.unet_in = unet_in.p; sa.ld_in = 64; sa.cloth_ch0 = 9 + pose_ch;
            sa.trace_eps = trace_eps; sa.trace_lat = trace_lat; sa.trace_cap = trace_cap;
            sa.step_noise = use_step_noise ? step_noise_buf : nullptr;
            sa.guidance_tab = guided ? d_gtab : nullptr;
            sa.factor = use_factor ? d_factor : nullptr;
            sa.pag_tab = pag_on ? d_pag : nullptr;
            if (keep_lat) { sa.keep_x0 = keep_x0; sa.keep_noise = keep_noise; sa.keep_mask = keep_mask; sa.keep_tab = d_keep_tab; }
            // the UNet forward runs as lanes.G independent sample groups on as many streams (runtime.h UNetLanes); the lanes own their
            // arenas, the shared noise prediction lives in this one
            const int eps_ld = (unet->cfg.out_channels + 3) / 4 * 4;
            Act eps = c.new_act(n, h, w, unet->cfg.out_channels, eps_ld);
            const size_t mk_loop = arena.mark();
            // cond: a cond-only evaluation of a guided run -- the UNet runs over the conditional samples [B, 2B) (their rows of unet_in and
            // eps, their part of the K/V cache) and the step kernel, told by the table, reads only those rows of eps
            // sh: a shallow evaluation (feature cache); a whole evaluation of a cached run captures
            // pg: a PAG evaluation -- the forward also runs over the perturbed group, the rows behind the cond group's, perturbed from sample
            // ng * B of the context batch.  In a PAG-shaped run an evaluation without PAG runs over the rows [0, ng * B) or [B, 2B): today's forms
            auto one_step = [&](bool concurrent, bool cond = false, bool sh = false, bool pg = false) {
                arena.release(mk_loop);
                FeatCache fcs; fcs.mode = sh ? FeatCache::SHALLOW : FeatCache::CAPTURE; fcs.branch = fc_branch; fcs.buf = fcache;
                const FeatCache* fc = fc_on ? &fcs : nullptr;
                if (pag_on) {
                    const int s0 = cond ? B : 0, ns = ((cond ? 1 : ng) + (pg ? 1 : 0)) * B;
                    Act xs = unet_in, es = eps;
                    xs.n = ns; xs.p = unet_in.p + (size_t)s0 * hw * unet_in.ld;
                    es.n = ns; es.p = eps.p + (size_t)s0 * hw * eps.ld;
                    lanes.forward(*unet, st, c.dry(), concurrent, xs, es, unet->temb_table, d_step, s0, fc, pg ? ng * B : (int)PAG_NONE);
                } else if (cond) {
                    Act xs = unet_in, es = eps;
                    xs.n = B; xs.p = unet_in.p + (size_t)B * hw * unet_in.ld;
                    es.n = B; es.p = eps.p + (size_t)B * hw * eps.ld;
                    lanes.forward(*unet, st, c.dry(), concurrent, xs, es, unet->temb_table, d_step, B, fc);
                } else lanes.forward(*unet, st, c.dry(), concurrent, unet_in, eps, unet->temb_table, d_step, 0, fc);
                if (c.dry()) return;
                sa.eps = eps.p; sa.ld_eps = eps.ld;
                if (use_factor && !cond)
                    c.check(pag_on ? ladi_launch_cfg_stats_pag(eps.p, eps.ld, B, hw, d_gtab, d_step, 0.f, d_pag, 0.f, phi, d_factor, st)
                                   : ladi_launch_cfg_stats(eps.p, eps.ld, B, hw, d_gtab, d_step, 0.f, phi, d_factor, st), "cfg_stats");
                c.check(ladi_launch_sched_step(sa, st), "sched_step");
            };
            // step callback after evaluation i (between launches, never inside a capture): latents out to the caller's NCHW buffer, the host
            // call, the buffer back into the loop and the next UNet input.  Work the callback queued on the caller's stream comes first.
            // A non-zero return of the callback lands in cb_rc and ends the loop (the run is then aborted).  No callback set: nothing is
            // launched and nothing waits.
            int cb_rc = 0, cb_eval = -1;
            auto callback_point = [&](int i) {
                if (!cb_fn || i % cb_every) return;
                c.check(ladi_launch_lat_pix_to_nchw(latents, B, hw, cb_latents, st), "callback export");
                HIP_OK(hipStreamSynchronize(st));
                cb_eval = i;
                if ((cb_rc = cb_fn(cb_user, i)) != 0) return;
                HIP_OK(hipEventRecord(ev_in, user_st));
                HIP_OK(hipStreamWaitEvent(st, ev_in, 0));
                c.check(ladi_launch_latents_import(cb_latents, B, hw, latents, unet_in.p, 64, cfgf, table[i].in_scale_next, st, pag_on ? 1 : 0),
                        "callback import");
            };
            // the forms of an evaluation: bit 0 cond-only, bit 1 shallow, bit 2 PAG (never with bit 1).  Which ones this run has, for the
            // planning pass
            auto form = [&](int i) { return (cond_only(i) ? 1 : 0) | (whole[i] ? 0 : 2) | (pag_eval(i) ? 4 : 0); };
            bool has_form[8] = {false, false, false, false, false, false, false, false};
            for (int i = 0; i < evals; ++i) has_form[form(i)] = true;
            // the first evaluation of any form runs its lanes one after the other (one-time function attribute setup, per-shape tile measurement)
            bool seen[8] = {false, false, false, false, false, false, false, false};
            // an evaluation whose forward ran over B samples (launched eagerly or by replaying the cond-only graph; every one of a run without CFG)
            auto ran = [&](int f) { if ((f & 1) || !cfgf) ++last_cond_only; if (f & 2) ++last_shallow; };
            if (c.dry()) {
                one_step(false);
                if (any_cond_only) one_step(false, true);
                if (has_form[2]) one_step(false, false, true);
                if (has_form[3]) one_step(false, true, true);
                if (has_form[4]) one_step(false, false, false, true);
                if (has_form[5]) one_step(false, true, false, true);
            }
            else if (!in.use_graph || evals < 3) {
                for (int i = 0; i < evals && !cb_rc; ++i) {
                    const int f = form(i);
                    one_step(i > 0 && seen[f], f & 1, f & 2, f & 4); seen[f] = true; ran(f);
                    callback_point(i);
                }
            } else {
                one_step(false, cond_only(0), false, pag_eval(0));  // eager first evaluation (always whole)
                seen[form(0)] = true; ran(form(0));
                callback_point(0);
                unsigned long long key = 0x1234;
                key = mix(key, (unsigned long long)(uintptr_t)arena.base); key = mix(key, (unsigned long long)B * 1000003ULL + H * 4099ULL + W);
                key = mix(key, (unsigned long long)cfgf); key = mix(key, (unsigned long long)L);
                unsigned gb = 0; if (!guided) std::memcpy(&gb, &in.guidance, 4);     // with a table the scalar is ignored: not part of the key
                key = mix(key, gb);
                key = mix(key, (unsigned long long)(uintptr_t)unet->temb_table); key = mix(key, (unsigned long long)(uintptr_t)unet->mid_xf.kv_cache);
                key = mix(key, (unsigned long long)(uintptr_t)d_table); key = mix(key, (unsigned long long)(uintptr_t)stats);
                key = mix(key, (unsigned long long)pose_ch * 7 + has_cloth);
                key = mix(key, (unsigned long long)(uintptr_t)trace_eps); key = mix(key, (unsigned long long)(uintptr_t)trace_lat);
                key = mix(key, (unsigned long long)trace_cap);
                key = mix(key, (unsigned long long)(uintptr_t)sa.step_noise);
                key = mix(key, lanes.key());
                // a graph captured without the probe launches is never replayed with it, nor one that holds another probe's slots: the id is
                // unique per Probe (0 = none), and within one Probe a name keeps its slot
                key = mix(key, unet->probe ? unet->probe->id : 0ULL);
                // both graphs (full and cond-only evaluation) live under one key, with the guidance table, the factor buffer and phi
                unsigned pb; std::memcpy(&pb, &phi, 4);
                key = mix(key, (unsigned long long)(uintptr_t)sa.guidance_tab); key = mix(key, (unsigned long long)(uintptr_t)sa.factor);
                key = mix(key, guided ? 0x100000000ULL | pb : 0ULL);
                // ... and with the feature cache: its buffer, the branch and whether whole evaluations capture (a graph captured with
                // capture on is never replayed for a plain run, nor the reverse)
                key = mix(key, fc_on ? (unsigned long long)(uintptr_t)fcache : 0ULL);
                key = mix(key, fc_on ? 0x200000000ULL | (unsigned long long)fc_branch : 0ULL);
                // ... and with the latent blend: its buffers, the coefficient table and the mode
                key = mix(key, (unsigned long long)(uintptr_t)sa.keep_x0); key = mix(key, (unsigned long long)(uintptr_t)sa.keep_noise);
                key = mix(key, (unsigned long long)(uintptr_t)sa.keep_mask); key = mix(key, (unsigned long long)(uintptr_t)sa.keep_tab);
                key = mix(key, keep_lat ? 0x400000000ULL | (unsigned long long)preserve_mode : 0ULL);
                // ... and with FreeU: on / off and the bits of the four factors the captured launches carry as arguments
                {
                    const FreeU& fu = unet->freeu;
                    const float fv[4] = {fu.s1, fu.s2, fu.b1, fu.b2};
                    key = mix(key, fu.on ? 0x800000000ULL : 0ULL);
                    for (int i = 0; i < 4; ++i) { unsigned fb = 0; if (fu.on) std::memcpy(&fb, &fv[i], 4); key = mix(key, fb); }
                }
                // ... and with PAG: whether the run has the third group, the scale table and the selected blocks (a graph captured with PAG
                // is never replayed without it, nor the reverse)
                key = mix(key, pag_on ? 0x1000000000ULL | (unsigned long long)unet->pag_mask : 0ULL);
                key = mix(key, (unsigned long long)(uintptr_t)sa.pag_tab);
                if (key != graph_key) {
                    if (gexec) { (void)hipGraphExecDestroy(gexec); gexec = nullptr; }
                    if (graph) { (void)hipGraphDestroy(graph); graph = nullptr; }
                    if (gexec_cond) { (void)hipGraphExecDestroy(gexec_cond); gexec_cond = nullptr; }
                    if (graph_cond) { (void)hipGraphDestroy(graph_cond); graph_cond = nullptr; }
                    for (auto& g : gexec_sh) if (g) { (void)hipGraphExecDestroy(g); g = nullptr; }
                    for (auto& g : graph_sh) if (g) { (void)hipGraphDestroy(g); g = nullptr; }
                    for (auto& g : gexec_pag) if (g) { (void)hipGraphExecDestroy(g); g = nullptr; }
                    for (auto& g : graph_pag) if (g) { (void)hipGraphDestroy(g); g = nullptr; }
                    graph_key = key;
                }
                hipGraph_t* const grs[6] = {&graph, &graph_cond, &graph_sh[0], &graph_sh[1], &graph_pag[0], &graph_pag[1]};
                hipGraphExec_t* const ges[6] = {&gexec, &gexec_cond, &gexec_sh[0], &gexec_sh[1], &gexec_pag[0], &gexec_pag[1]};
                auto capture = [&](int f) {
                    hipGraph_t& gr = *grs[f];
                    hipGraphExec_t& ge = *ges[f];
                    if (gr) { (void)hipGraphDestroy(gr); gr = nullptr; }     // left by a capture whose instantiation failed
                    HIP_OK(hipStreamBeginCapture(st, hipStreamCaptureModeRelaxed));
                    try { one_step(true, f & 1, f & 2, f & 4); } catch (...) { hipGraph_t g = nullptr; (void)hipStreamEndCapture(st, &g); if (g) (void)hipGraphDestroy(g); throw; }
                    HIP_OK(hipStreamEndCapture(st, &gr));
                    HIP_OK(hipGraphInstantiate(&ge, gr, nullptr, nullptr, 0));
                };
                // the host knows the schedule and picks the graph; the values come from the device table.  A form that this run has not yet
                // run eagerly and that has no graph runs eagerly once (see above), its next evaluation captures
                for (int i = 1; i < evals && !cb_rc; ++i) {
                    const int f = form(i);
                    hipGraphExec_t& ge = *ges[f];
                    if (!ge && !seen[f]) { one_step(false, f & 1, f & 2, f & 4); seen[f] = true; }
                    else {
                        if (!ge) capture(f);
                        HIP_OK(hipGraphLaunch(ge, st));
                    }
                    ran(f);
                    callback_point(i);
                }
            }
            arena.release(mk_loop);
            if (cb_rc) {
                // the handle stays usable: the next run re-arms the step counter and the arrival ticket (hipMemsetAsync above)
                set_error("tryon: the step callback returned " + std::to_string(cb_rc) + " after evaluation " + std::to_string(cb_eval) +
                          ": run aborted");
                ev_valid = false;
                HIP_OK(hipEventRecord(ev_out, st));
                HIP_OK(hipStreamWaitEvent(user_st, ev_out, 0));
                return TRYON_CALLBACK_ABORT;
            }
            if (!c.dry()) HIP_OK(hipEventRecord(ev[2], st));
            // ---------------- 11. decode (tryon_pipe.py:349-359)
            {
                Act z = c.new_act(B, h, w, 64);
                // pixel composite with a feathered mask: the blurred mask and the row pass's scratch
                const bool feather = keep_pix && preserve_sigma > 0.f;
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
                    (void)vae->decode(c, z, use_emasc ? skips : nullptr, vae->range_shift < 0 ? 4 : vae->range_shift);
                } else {
                    // ONE decode at the guard's current shift; the flag is examined without a host round trip (runtime.h VAE::post_overflow_check /
                    // poll_overflow: at the entry of the next run, or by ladi_tryon_poll_overflow)
                    const int sh = vae->guard_shift();
                    arena.release(mk_dec);
                    c.stats_off = 0;
                    if (stats_cap) HIP_OK(hipMemsetAsync(stats, 0, stats_cap * sizeof(float), st));
                    Act img = vae->decode(c, z, use_emasc ? skips : nullptr, sh);
                    if (keep_pix) {
                        if (feather) c.check(ladi_launch_mask_feather(mask_bin, B, H, W, preserve_sigma, m_tmp, m_soft, st), "mask_feather");
                        c.check(ladi_launch_image_composite(img.p, img.ld, in.image, in.in_f32, feather ? (const void*)m_soft : (const void*)mask_bin,
                                                            feather ? 1 : 0, B, H * W, images_out, images_u8, st), "image_composite");
                    } else c.check(ladi_launch_image_post(img.p, img.ld, B * H * W, images_out, images_u8, st), "image_post");
                    vae->last_shift = sh;
                    vae->post_overflow_check(st);
                    if (latents_out) c.check(ladi_launch_lat_pix_to_nchw(latents, B, hw, latents_out, st), "latents_out");
                    HIP_OK(hipEventRecord(ev[3], st));
                    ev_valid = true;
                }
            }
            if (pass == 0) {
                lanes.commit_plan();
                commit_plan(arena, c.stats_peak, &stats, &stats_cap);
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
    return rc;
}

}  // namespace ladi
