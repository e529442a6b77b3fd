// Extended SD2-inpainting UNet (31 input channels) forward on the native kernels.
// Architecture restated in SURVEY.md App. A.1-A.3 (diffusers 0.14.0 UNet2DConditionModel as configured by the
// reference at hubconf.py:31-39 and called at src/vto_pipelines/tryon_pipe.py:732).
#include "runtime.h"
#include <stdexcept>
#include <cstring>
#include <new>
#include <cstdlib>
#include <cstdio>
#include <cmath>

namespace ladi {

#define HIP_OK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) throw std::runtime_error(std::string(#x) + ": " + hipGetErrorString(e_)); } while (0)

static ResBlock load_res(DevPool& pool, const WeightStore& ws, const std::string& p, bool temb) {
    ResBlock r;
    r.n1 = load_norm(pool, ws, p + ".norm1");
    r.c1 = load_conv(pool, ws, p + ".conv1");
    r.n2 = load_norm(pool, ws, p + ".norm2");
    r.c2 = load_conv(pool, ws, p + ".conv2");
    r.cin = r.c1.cin; r.cout = r.c1.cout;
    r.has_sc = ws.has(p + ".conv_shortcut.weight");
    if (r.has_sc) r.sc = load_conv(pool, ws, p + ".conv_shortcut");
    (void)temb;
    return r;
}

static XfBlock load_xf(DevPool& pool, const WeightStore& ws, const std::string& p, int heads, bool pack_fused) {
    XfBlock x;
    x.gn = load_norm(pool, ws, p + ".norm");
    x.proj_in = load_conv(pool, ws, p + ".proj_in");
    const std::string b = p + ".transformer_blocks.0";
    x.ln1 = load_norm(pool, ws, b + ".norm1");
    x.ln2 = load_norm(pool, ws, b + ".norm2");
    x.ln3 = load_norm(pool, ws, b + ".norm3");
    x.qkv = load_linear_cat(pool, ws, {b + ".attn1.to_q", b + ".attn1.to_k", b + ".attn1.to_v"}, false);
    x.o1 = load_conv(pool, ws, b + ".attn1.to_out.0");
    x.q2 = load_conv(pool, ws, b + ".attn2.to_q");
    x.kv2 = load_linear_cat(pool, ws, {b + ".attn2.to_k", b + ".attn2.to_v"}, false);
    x.o2 = load_conv(pool, ws, b + ".attn2.to_out.0");
    x.ff1 = load_geglu(pool, ws, b + ".ff.net.0.proj");
    x.ff2 = load_conv(pool, ws, b + ".ff.net.2");
    x.proj_out = load_conv(pool, ws, p + ".proj_out");
    x.C = x.proj_in.cout;
    x.heads = heads;
    if (x.C != heads * 64) throw std::runtime_error(p + ": head_dim must be 64");
    // the C = 320 level CAN run attn2 and the feed-forward as fused kernels (xf_fused.hip, default off): pack to_out / ff.net.2 per head / per
    // hidden block -- only when the path is switched on (UNet::xf_fuse): the default path reads none of it
    if (pack_fused && ladi_xf_fused_eligible(x.C, heads, 128, 1) && x.o2.cin_pad == x.C && x.ff2.cin_pad == 4 * x.C && x.ff1.cout == 8 * x.C) {
        x.o2_packed = reinterpret_cast<h16*>(pool.alloc(ladi_xf_wo_packed_elems() * sizeof(h16)));
        x.ff2_packed = reinterpret_cast<h16*>(pool.alloc(ladi_xf_w2_packed_elems() * sizeof(h16)));
        if (ladi_launch_pack_wo(x.o2.w, x.o2_packed, nullptr) || ladi_launch_pack_w2(x.ff2.w, x.ff2_packed, nullptr) || hipDeviceSynchronize() != hipSuccess)
            throw std::runtime_error(p + ": packing the fused-block operands failed");
    }
    return x;
}

void UNet::load(const UNetCfg& c, const WeightStore& ws) {
    cfg = c;
    // LADI_XF_FUSE (0 / 1 / 2: none / attn2 only / attn2 + feed-forward as fused kernels) is latched HERE, once per UNet: the value selects
    // different arena allocations in the forward, so a planning pass, its real pass, a later re-plan and the lanes of one forward must all
    // see the same one (it used to be a getenv in every block of every pass)
    { const char* e = getenv("LADI_XF_FUSE"); xf_fuse = e ? atoi(e) : 0; }
    const int L = c.layers_per_block;
    conv_in = load_conv(pool, ws, "conv_in", c.in_channels);
    time_l1 = load_conv(pool, ws, "time_embedding.linear_1");
    time_l2 = load_conv(pool, ws, "time_embedding.linear_2");
    std::vector<std::string> temb_names;
    auto add_res = [&](std::vector<ResBlock>* vec, ResBlock* single, const std::string& p) {
        ResBlock r = load_res(pool, ws, p, true);
        r.temb_off = temb_total;
        temb_total += r.cout;
        temb_names.push_back(p + ".time_emb_proj");
        if (vec) vec->push_back(r); else *single = r;
    };
    // the transformer blocks are loaded in execution order: this is the one place that says which block has which bit, level and prefix.
    // A second load() starts the table again.  The reserve is a hint only: nothing points into the table before build_lora_targets()
    xf.clear(); xf.reserve(6 * L + 4);
    auto add_xf = [&](const std::string& p, int level) {
        XfBlock x = load_xf(pool, ws, p, c.heads[level], xf_fuse > 0);
        x.bit = (int)xf.size(); x.level = level; x.prefix = p;
        xf.push_back(std::move(x));
    };
    for (int i = 0; i < 4; ++i) {
        for (int j = 0; j < L; ++j) {
            const std::string p = "down_blocks." + std::to_string(i);
            add_res(&down_res, nullptr, p + ".resnets." + std::to_string(j));
            if (i < 3) add_xf(p + ".attentions." + std::to_string(j), i);
        }
        if (i < 3) down_samp[i] = load_conv(pool, ws, "down_blocks." + std::to_string(i) + ".downsamplers.0.conv");
    }
    add_res(nullptr, &mid_res[0], "mid_block.resnets.0");
    add_xf("mid_block.attentions.0", 3);
    pag_mask = 1u << xf.back().bit;         // pag_applied_layers defaults to the mid block
    mid_bit = xf.back().bit;
    add_res(nullptr, &mid_res[1], "mid_block.resnets.1");
    for (int i = 0; i < 4; ++i) {
        for (int j = 0; j < L + 1; ++j) {
            const std::string p = "up_blocks." + std::to_string(i);
            add_res(&up_res, nullptr, p + ".resnets." + std::to_string(j));
            if (i > 0) add_xf(p + ".attentions." + std::to_string(j), 3 - i);
        }
        if (i < 3) up_samp[i] = load_conv(pool, ws, "up_blocks." + std::to_string(i) + ".upsamplers.0.conv");
    }
    norm_out = load_norm(pool, ws, "conv_norm_out");
    conv_out = load_conv(pool, ws, "conv_out");
    temb_all = load_linear_cat(pool, ws, temb_names, true);
    build_lora_targets();
}

UNet::~UNet() {
    if (temb_table) (void)hipFree(temb_table);
    if (stats) (void)hipFree(stats);
    if (in_buf) (void)hipFree(in_buf);
    if (fc_buf) (void)hipFree(fc_buf);
    for (auto& l : tome.lv) if (l.mem) (void)hipFree(l.mem);
    if (sag_mem) (void)hipFree(sag_mem);
}

// ------------------------------------------------------------------------------------------------
// Self-attention guidance map (runtime.h UNet::sag_capture; sag.hip)
// ------------------------------------------------------------------------------------------------
void UNet::sag_prepare(int T, int need_n, bool dry) {
    if (sag_cap_n >= need_n && sag_cap_T >= T) { if (dry) sag_T = T; return; }
    if (!dry) throw std::runtime_error("SAG map: no planning pass has seen " + std::to_string(need_n) + " samples of " + std::to_string(T) + " tokens");
    const int cn = need_n > sag_cap_n ? need_n : sag_cap_n, cT = T > sag_cap_T ? T : sag_cap_T;
    if (sag_mem) { HIP_OK(hipDeviceSynchronize()); (void)hipFree(sag_mem); }
    sag_mem = nullptr; sag_s = nullptr; sag_m = nullptr; sag_cap_n = sag_cap_T = 0;
    const size_t fl = ((size_t)cn * cT * sizeof(float) + 255) & ~(size_t)255, by = ((size_t)cn * cT + 255) & ~(size_t)255;
    HIP_OK(hipMalloc(&sag_mem, fl + by));
    HIP_OK(hipMemset(sag_mem, 0, fl + by));
    sag_s = reinterpret_cast<float*>(sag_mem); sag_m = reinterpret_cast<unsigned char*>(sag_mem) + fl;
    sag_cap_n = cn; sag_cap_T = cT; sag_T = T;
}

// ------------------------------------------------------------------------------------------------
// Token merging (runtime.h ToMe; tome.hip)
// ------------------------------------------------------------------------------------------------
std::string tome_cfg_error(const ToMeCfg& c) {
    if (!std::isfinite(c.ratio) || c.ratio < 0.0 || c.ratio >= 1.0) return "ratio " + std::to_string(c.ratio) + " is outside [0, 1) or not finite";
    if (c.sx != 2 || c.sy != 2) return "sx = " + std::to_string(c.sx) + ", sy = " + std::to_string(c.sy) + ": only 2 x 2 cells are supported";
    if (c.max_downsample != 1 && c.max_downsample != 2) return "max_downsample " + std::to_string(c.max_downsample) + " is not 1 or 2";
    if (c.ratio > 0.0 && !c.merge_attn && !c.merge_crossattn && !c.merge_mlp) return "merge_attn, merge_crossattn and merge_mlp are all off with ratio > 0";
    return std::string();
}

void UNet::tome_set(const ToMeCfg* c) {
    ToMeCfg n;
    if (c) {
        const std::string e = tome_cfg_error(*c);
        if (!e.empty()) throw std::runtime_error(e);
        n = *c;
        n.use_rand = c->use_rand ? 1 : 0; n.merge_attn = c->merge_attn ? 1 : 0; n.merge_crossattn = c->merge_crossattn ? 1 : 0; n.merge_mlp = c->merge_mlp ? 1 : 0;
    }
    // a forward still in flight reads the tables and writes the out_row buffers
    if (tome.lv[0].mem || tome.lv[1].mem) HIP_OK(hipDeviceSynchronize());
    for (auto& l : tome.lv) { if (l.mem) (void)hipFree(l.mem); l = ToMeLevel(); }
    for (auto& p : tome.out_row) p = nullptr;
    tome.cfg = n;
    tome.on = c && n.ratio > 0.0;
    ++tome.gen;
}

std::vector<int> UNet::tome_blocks() const {
    std::vector<int> v;
    if (!tome.on) return v;
    for (auto& b : xf)
        if (b.level < tome.cfg.max_downsample) v.push_back(b.bit);
    return v;
}

const ToMeLevel* UNet::tome_prepare(int level, int h, int w, int need_n, bool dry) {
    ToMeLevel& l = tome.lv[level];
    if (l.h == h && l.w == w && l.cap_n >= need_n) return &l;
    if (!dry) throw std::runtime_error("token merging: no planning pass has seen " + std::to_string(need_n) + " samples of " + std::to_string(h) + " x " +
                                       std::to_string(w) + " tokens on level " + std::to_string(level));
    const ToMeCfg& c = tome.cfg;
    ToMeLevel nl;
    nl.h = h; nl.w = w; nl.T = h * w; nl.cap_n = need_n;
    nl.Nd = ladi_tome_tables_host(h, w, c.sx, c.sy, c.use_rand, c.seed, nullptr, nullptr, 0);
    if (nl.Nd < 0) throw std::runtime_error("token merging: " + std::to_string(h) + " x " + std::to_string(w) + " tokens cannot be partitioned");
    nl.Ns = nl.T - nl.Nd;
    nl.r = nl.Nd > 0 ? ladi_tome_count_host(nl.T, nl.Ns, c.ratio) : 0;
    if (nl.r > 0 && nl.Nd > 4096)
        throw std::runtime_error("token merging: " + std::to_string(h) + " x " + std::to_string(w) + " tokens give " + std::to_string(nl.Nd) +
                                 " dst tokens, the plan kernel holds at most 4096");
    std::vector<int> bits;
    for (auto& b : xf) if (b.level == level && b.bit < 32) bits.push_back(b.bit);
    if (l.mem) { HIP_OK(hipDeviceSynchronize()); (void)hipFree(l.mem); }
    l = ToMeLevel();
    for (int b : bits) tome.out_row[b] = nullptr;
    ++tome.gen;
    if (nl.r > 0) {
        auto up = [](size_t ints) { return (ints * sizeof(int) + 255) & ~(size_t)255; };
        const size_t tab = up((size_t)nl.Ns) + up((size_t)nl.Nd), rows = up((size_t)need_n * nl.T);
        HIP_OK(hipMalloc(&nl.mem, tab + rows * bits.size()));
        char* p = reinterpret_cast<char*>(nl.mem);
        nl.src_pos = reinterpret_cast<int*>(p); nl.dst_pos = reinterpret_cast<int*>(p + up((size_t)nl.Ns));
        std::vector<int> sp((size_t)nl.T), dp((size_t)nl.T);
        (void)ladi_tome_tables_host(h, w, c.sx, c.sy, c.use_rand, c.seed, sp.data(), dp.data(), nl.T);
        hipError_t e = hipMemcpy(nl.src_pos, sp.data(), (size_t)nl.Ns * sizeof(int), hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemcpy(nl.dst_pos, dp.data(), (size_t)nl.Nd * sizeof(int), hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemset(p + tab, 0, rows * bits.size());
        if (e != hipSuccess) { (void)hipFree(nl.mem); throw std::runtime_error(std::string("token merging: table upload: ") + hipGetErrorString(e)); }
        for (size_t k = 0; k < bits.size(); ++k) tome.out_row[bits[k]] = reinterpret_cast<int*>(p + tab + rows * k);
    }
    l = nl;
    return &l;
}

int UNet::set_context(const h16* ehs, int n, int L, hipStream_t st) {
    // cross-attention K/V of every transformer block depend only on encoder_hidden_states: hoisted out of the
    // denoising loop (SURVEY.md §8d "step-invariant work")
    if (n * L > ctx_cap_n || n > ctx_cap_samples) {
        ctx_pool.reset(new DevPool());   // frees the previous (smaller) K/V cache
        for (auto& x : xf) {
            x.kv_cache = reinterpret_cast<h16*>(ctx_pool->alloc((size_t)n * L * 2 * x.C * sizeof(h16)));
            if (x.o2_packed) {
                x.kp_tiles = reinterpret_cast<h16*>(ctx_pool->alloc(ladi_xf_kp_elems(n) * sizeof(h16)));
                x.vt_tiles = reinterpret_cast<h16*>(ctx_pool->alloc(ladi_xf_vt_elems(n) * sizeof(h16)));
            }
        }
        ctx_cap_n = n * L; ctx_cap_samples = n;
    }
    ctx_n = n; ctx_L = L;
    fc_rows.assign((size_t)n, 0);            // the stand-alone entry's deep-feature cache belongs to the context it was captured under
    for (auto& x : xf) {
        IGemmArgs a; std::memset(&a, 0, sizeof(a));
        a.src0 = ehs; a.C0 = cfg.cross_dim; a.ld0 = cfg.cross_dim;
        a.Hs = n * L; a.Ws = 1; a.Ho = n * L; a.Wo = 1; a.P = n * L;
        a.ksize = 1; a.stride = 1; a.pad = 0;
        a.W = x.kv2.w; a.Q = x.kv2.cout; a.K = x.kv2.K();
        a.out = x.kv_cache; a.ldo = 2 * x.C; a.out_scale = 1.f;
        int rc = ladi_launch_igemm(a, 1, 0, st);
        if (rc) { set_error("set_context igemm rc=" + std::to_string(rc)); return rc; }
        if (x.kp_tiles && ladi_xf_fused_eligible(x.C, x.heads, 128, L)) {      // the fused attn2 reads per-(sample, head) tiles
            rc = ladi_launch_pack_kv_tiles(x.kv_cache, n, L, x.C, x.kp_tiles, x.vt_tiles, st);
            if (rc) { set_error("set_context pack_kv_tiles rc=" + std::to_string(rc)); return rc; }
        }
    }
    return 0;
}

int UNet::compute_temb(const float* ts_host, int count, hipStream_t st) {
    const int tdim = time_l1.cout;   // 1280
    const int edim = time_l1.cin;    // 320
    if (count > temb_rows_cap) {
        if (temb_table) (void)hipFree(temb_table);
        HIP_OK(hipMalloc(reinterpret_cast<void**>(&temb_table), (size_t)count * (temb_total + 2 * tdim + edim + 1) * sizeof(float)));
        temb_rows_cap = count;
    }
    float* table = temb_table;                               // [count][temb_total]
    float* t_dev = table + (size_t)temb_rows_cap * temb_total;  // [count]
    float* emb0 = t_dev + temb_rows_cap;                     // [count][edim]
    float* h1 = emb0 + (size_t)temb_rows_cap * edim;         // [count][tdim]
    float* h2 = h1 + (size_t)temb_rows_cap * tdim;           // [count][tdim]
    HIP_OK(hipMemcpyAsync(t_dev, ts_host, (size_t)count * sizeof(float), hipMemcpyHostToDevice, st));
    int rc = ladi_launch_timestep_embedding(t_dev, count, edim, emb0, st);
    // reference casts the sinusoid to the model dtype (fp16) before linear_1; keep fp32 (more accurate)
    if (!rc) rc = ladi_launch_small_linear(emb0, 1, edim, time_l1.w, time_l1.b, nullptr, 0, count, tdim, time_l1.cin_pad, LADI_ACT_SILU, 0, h1, 1, tdim, st);
    if (!rc) rc = ladi_launch_small_linear(h1, 1, tdim, time_l2.w, time_l2.b, nullptr, 0, count, tdim, time_l2.cin_pad, LADI_ACT_NONE, 0, h2, 1, tdim, st);
    if (!rc) rc = ladi_launch_small_linear(h2, 1, tdim, temb_all.w, temb_all.b, nullptr, 0, count, temb_total, temb_all.cin_pad, LADI_ACT_NONE, 1, table, 1, temb_total, st);
    temb_rows = count;
    if (rc) set_error("compute_temb rc=" + std::to_string(rc));
    return rc;
}

// ------------------------------------------------------------------------------------------------
// IP-Adapter image prompt (runtime.h UNet; ip_adapter.hip)
// ------------------------------------------------------------------------------------------------
// the weights of ip_load with a Resampler as image_proj.* (Plus): validated by Resampler::load, K/V weights as for the plain adapter
static void ip_load_plus(UNet& u, const WeightStore& ws, int dim_head) {
    const int D = u.cfg.cross_dim;
    for (auto& kv : ws.m) {
        const std::string& k = kv.first;
        bool known = k.compare(0, 11, "image_proj.") == 0;
        for (auto& b : u.xf)
            known = known || k == b.prefix + ".transformer_blocks.0.attn2.processor.to_k_ip.weight" ||
                    k == b.prefix + ".transformer_blocks.0.attn2.processor.to_v_ip.weight";
        if (!known) throw std::runtime_error("unexpected key '" + k + "'");
    }
    for (auto& b : u.xf)
        for (const char* nm : {"to_k_ip", "to_v_ip"}) {
            const std::string k = b.prefix + ".transformer_blocks.0.attn2.processor." + nm + ".weight";
            if (!ws.has(k)) throw std::runtime_error("'" + k + "' is missing");
            const HostTensor& w = ws.get(k);
            if (w.shape.size() != 2 || w.shape[0] != b.C || w.shape[1] != D)
                throw std::runtime_error(k + " is not [" + std::to_string(b.C) + ", " + std::to_string(D) + "]");
        }
    std::unique_ptr<Resampler> rs(new Resampler());
    rs->check(ws, "image_proj.", dim_head);       // host only; the device is touched after the last refusal
    if (rs->out_dim != D)
        throw std::runtime_error("the Resampler's output width " + std::to_string(rs->out_dim) + " is not the UNet's cross-attention width " + std::to_string(D));
    rs->upload(ws, "image_proj.");
    std::unique_ptr<DevPool> pool_(new DevPool());
    std::vector<DConv> kv;
    for (auto& b : u.xf) {
        const std::string p = b.prefix + ".transformer_blocks.0.attn2.processor.";
        kv.push_back(load_linear_cat(*pool_, ws, {p + "to_k_ip", p + "to_v_ip"}, false));
    }
    HIP_OK(hipDeviceSynchronize());
    for (auto& b : u.xf) { b.ip_kv = kv[b.bit]; b.ip_scale = 1.f; }
    u.ip_pool = std::move(pool_);
    u.ip_proj_w = u.ip_proj_b = nullptr; u.ip_norm = DNorm();
    u.ip_N = rs->N; u.ip_E = rs->E; u.ip_dim_head = dim_head;
    u.ip_resampler = std::move(rs);
    u.ip_loaded = true;
    u.ip_ctx_n = 0;
}

void UNet::ip_load(const WeightStore& ws, int dim_head) {
    if (ip_loaded) throw std::runtime_error("an IP-Adapter is already loaded (ladi_unet_ip_adapter_unload first)");
    if (ws.has("image_proj.latents")) { ip_load_plus(*this, ws, dim_head); return; }
    auto shape_str = [](const HostTensor& t) { std::string s = "["; for (size_t i = 0; i < t.shape.size(); ++i) s += (i ? ", " : "") + std::to_string(t.shape[i]); return s + "]"; };
    auto need = [&](const std::string& k) -> const HostTensor& {
        if (!ws.has(k)) throw std::runtime_error("'" + k + "' is missing");
        return ws.get(k);
    };
    // ---- validate everything; nothing of the UNet changes before the end of this block
    const int D = cfg.cross_dim;
    const HostTensor& pw = need("image_proj.proj.weight");
    if (pw.shape.size() != 2 || pw.shape[0] < D || pw.shape[0] % D || pw.shape[1] < 1)
        throw std::runtime_error("image_proj.proj.weight of shape " + shape_str(pw) + " is not [N * " + std::to_string(D) + ", E]");
    const long long N = pw.shape[0] / D, E = pw.shape[1];
    if (N < 1 || N > 64) throw std::runtime_error("image_proj.proj.weight gives " + std::to_string(N) + " image tokens, outside [1, 64]");
    if (E % 8) throw std::runtime_error("the image embedding width " + std::to_string(E) + " is not a multiple of 8");
    if ((long long)need("image_proj.proj.bias").numel() != N * D) throw std::runtime_error("image_proj.proj.bias does not have " + std::to_string(N * D) + " entries");
    if ((long long)need("image_proj.norm.weight").numel() != D || (long long)need("image_proj.norm.bias").numel() != D)
        throw std::runtime_error("image_proj.norm does not have " + std::to_string(D) + " channels");
    size_t expected = 4;
    for (auto& b : xf) {
        for (const char* nm : {"to_k_ip", "to_v_ip"}) {
            const std::string k = b.prefix + ".transformer_blocks.0.attn2.processor." + nm + ".weight";
            const HostTensor& w = need(k);
            if (w.shape.size() != 2 || w.shape[0] != b.C || w.shape[1] != D)
                throw std::runtime_error(k + " of shape " + shape_str(w) + " is not [" + std::to_string(b.C) + ", " + std::to_string(D) + "]");
            ++expected;
        }
        if (ws.has(b.prefix + ".transformer_blocks.0.attn2.processor.to_k_ip.bias") || ws.has(b.prefix + ".transformer_blocks.0.attn2.processor.to_v_ip.bias"))
            throw std::runtime_error(b.prefix + ": to_k_ip / to_v_ip have no bias");
    }
    if (ws.m.size() != expected) {
        for (auto& kv : ws.m) {
            const std::string& k = kv.first;
            bool known = k == "image_proj.proj.weight" || k == "image_proj.proj.bias" || k == "image_proj.norm.weight" || k == "image_proj.norm.bias";
            for (auto& b : xf)
                known = known || k == b.prefix + ".transformer_blocks.0.attn2.processor.to_k_ip.weight" ||
                        k == b.prefix + ".transformer_blocks.0.attn2.processor.to_v_ip.weight";
            if (!known) throw std::runtime_error("unexpected key '" + k + "'");
        }
    }
    // ---- load
    std::unique_ptr<DevPool> pool_(new DevPool());
    h16* w = pool_->upload_h16(pw.data);
    h16* bias = pool_->upload_h16(ws.get("image_proj.proj.bias").data);
    DNorm nm = load_norm(*pool_, ws, "image_proj.norm");
    std::vector<DConv> kv;
    for (auto& b : xf) {
        const std::string p = b.prefix + ".transformer_blocks.0.attn2.processor.";
        kv.push_back(load_linear_cat(*pool_, ws, {p + "to_k_ip", p + "to_v_ip"}, false));
    }
    HIP_OK(hipDeviceSynchronize());
    for (auto& b : xf) { b.ip_kv = kv[b.bit]; b.ip_scale = 1.f; }
    ip_pool = std::move(pool_);
    ip_proj_w = w; ip_proj_b = bias; ip_norm = nm;
    ip_N = (int)N; ip_E = (int)E; ip_loaded = true;
    ip_ctx_n = 0;
}

void UNet::ip_unload() {
    ip_ctx_n = 0; ip_ctx_N = 0; ip_ctx_cap = 0;
    for (auto& b : xf) { b.ip_kv = DConv(); b.ip_kv_cache = nullptr; b.ip_scale = 1.f; }
    ip_lin = ip_tok = nullptr;
    ip_ctx_pool.reset();
    ip_pool.reset();
    ip_resampler.reset();
    ip_proj_w = ip_proj_b = nullptr; ip_norm = DNorm();
    ip_N = ip_E = 0; ip_loaded = false;
}

void UNet::ip_set_scale(const float* scales, int count) {
    if (!ip_loaded) throw std::runtime_error("no IP-Adapter is loaded (ladi_unet_ip_adapter_load)");
    if (!scales || count != pag_layer_count())
        throw std::runtime_error("want " + std::to_string(pag_layer_count()) + " scales, one per transformer block, but got " + std::to_string(count));
    for (int i = 0; i < count; ++i)
        if (!std::isfinite(scales[i])) throw std::runtime_error("scale " + std::to_string(i) + " is not finite");
    for (auto& b : xf) b.ip_scale = scales[b.bit];
}

void UNet::ip_reserve(int n, int N) {
    if (!ip_loaded) throw std::runtime_error("no IP-Adapter is loaded (ladi_unet_ip_adapter_load)");
    if (n < 1 || N < 1 || N > 64) throw std::runtime_error("image context of " + std::to_string(n) + " samples x " + std::to_string(N) + " tokens: n >= 1 and N in [1, 64]");
    const size_t rows = (size_t)n * N;
    if (rows > ip_ctx_cap) {
        ip_ctx_pool.reset(new DevPool());   // frees the previous (smaller) image K/V
        const size_t D = (size_t)cfg.cross_dim;
        ip_lin = reinterpret_cast<h16*>(ip_ctx_pool->alloc(rows * D * sizeof(h16)));
        ip_tok = reinterpret_cast<h16*>(ip_ctx_pool->alloc(rows * D * sizeof(h16)));
        for (auto& b : xf) b.ip_kv_cache = reinterpret_cast<h16*>(ip_ctx_pool->alloc(rows * 2 * b.C * sizeof(h16)));
        ip_ctx_cap = rows;
    }
    ip_ctx_n = n; ip_ctx_N = N;
}

// the image K/V of every block from the tokens in ip_tok: one igemm per block, as set_context's
static int ip_project_kv(UNet& u, const h16* tok, hipStream_t st) {
    const int rows = u.ip_ctx_n * u.ip_ctx_N;
    for (auto& x : u.xf) {
        IGemmArgs a; std::memset(&a, 0, sizeof(a));
        a.src0 = tok; a.C0 = u.cfg.cross_dim; a.ld0 = u.cfg.cross_dim;
        a.Hs = rows; a.Ws = 1; a.Ho = rows; a.Wo = 1; a.P = rows;
        a.ksize = 1; a.stride = 1; a.pad = 0;
        a.W = x.ip_kv.w; a.Q = x.ip_kv.cout; a.K = x.ip_kv.K();
        a.out = x.ip_kv_cache; a.ldo = 2 * x.C; a.out_scale = 1.f;
        const int rc = ladi_launch_igemm(a, 1, 0, st);
        if (rc) { u.ip_ctx_n = 0; set_error("set_ip_context igemm rc=" + std::to_string(rc)); return rc; }
    }
    return 0;
}

int UNet::set_ip_context(const h16* embeds, int n, hipStream_t st) {
    if (!embeds) throw std::runtime_error("null image embeddings");
    if (ip_resampler)
        throw std::runtime_error("the loaded IP-Adapter is a Plus adapter (Resampler): it takes hidden states [n][T][" + std::to_string(ip_E) +
                                 "] through ladi_unet_set_ip_context_seq, not one embedding per image");
    ip_reserve(n, ip_N);
    const int D = cfg.cross_dim;
    // tokens = LayerNorm(Linear(embeds)).reshape(n, N, cross_dim): the projection's output row [N * D] is N token rows of D
    int rc = ladi_launch_small_linear(embeds, 0, ip_E, ip_proj_w, ip_proj_b, nullptr, 0, n, ip_N * D, ip_E, LADI_ACT_NONE, 0, ip_lin, 0, ip_N * D, st);
    if (!rc) rc = ladi_launch_layernorm(ip_lin, D, ip_norm.g, ip_norm.b, 1e-5f, n * ip_N, D, ip_tok, D, st);
    if (rc) { ip_ctx_n = 0; set_error("set_ip_context image projection rc=" + std::to_string(rc)); return rc; }
    return ip_project_kv(*this, ip_tok, st);
}

int UNet::set_ip_context_seq(const h16* hidden, int n, int T, hipStream_t st) {
    if (!hidden) throw std::runtime_error("null hidden states");
    if (!ip_loaded) throw std::runtime_error("no IP-Adapter is loaded (ladi_unet_ip_adapter_load)");
    if (!ip_resampler)
        throw std::runtime_error("the loaded IP-Adapter is a plain adapter (Linear + LayerNorm projection): it takes one embedding per image "
                                 "through ladi_unet_set_ip_context, not a sequence of hidden states");
    if (T < 1) throw std::runtime_error("hidden states of " + std::to_string(T) + " tokens: T >= 1");
    ip_reserve(n, ip_N);
    try { ip_resampler->forward(hidden, n, T, ip_tok, st); }
    catch (...) { ip_ctx_n = 0; throw; }
    return ip_project_kv(*this, ip_tok, st);
}

int UNet::set_ip_tokens(const h16* tokens, int n, int N, hipStream_t st) {
    if (!tokens) throw std::runtime_error("null image tokens");
    ip_reserve(n, N);
    return ip_project_kv(*this, tokens, st);
}

namespace {

struct Fwd {
    Ctx& c; UNet& u; const float* temb; const int* tidx; int sample0;
    int pag_first = PAG_NONE;   // context index of the first perturbed sample (PAG)
    bool sag = false;           // this forward captures the SAG map (runtime.h UNet::sag_capture)
    Act res(const ResBlock& r, const Act& x, const Act* x2) {
        Act out;
        // block output is allocated first so temporaries can be released (stack discipline)
        out = new_act_with_stats(c, x.n, x.h, x.w, r.cout);
        const size_t mk = c.ar->mark();
        Act s1 = group_norm(c, r.n1, x, x2, u.cfg.groups, u.cfg.eps, 1);
        ConvOpt o1; o1.stats = true; o1.rowadd = temb + r.temb_off; o1.rowadd_idx = tidx; o1.rowadd_stride = u.temb_total;
        Act h1 = conv2d(c, r.c1, s1, nullptr, o1);
        Act s2 = group_norm(c, r.n2, h1, nullptr, u.cfg.groups, u.cfg.eps, 1);
        Act sc;
        const Act* resid = &x;
        if (r.has_sc) { ConvOpt os; sc = conv2d(c, r.sc, x, x2, os); resid = &sc; }
        else if (x2) throw std::runtime_error("resnet: concat input requires conv_shortcut");
        ConvOpt o2; o2.res0 = resid; o2.dst = &out;
        (void)conv2d(c, r.c2, s2, nullptr, o2);
        c.ar->release(mk);
        return out;
    }
    // np: the last np of the n samples are perturbed (PAG): the attention runs over the first n - np (one workgroup per (sample, head,
    // query tile): the others' results do not depend on n), the perturbed rows of o are the rows of v themselves
    Act attn(const h16* q, int ldq, long long sq, const h16* k, const h16* v, int ldkv, long long skv, int n, int T, int Nk,
             int heads, int np = 0) {
        Act o = c.new_act(n, T, 1, heads * 64);
        if (c.dry()) return o;
        if (np > 0) {
            const long long row0 = (long long)(n - np) * T;
            c.check(ladi_launch_pag_identity(v + row0 * ldkv, ldkv, o.p + row0 * o.ld, o.ld, (long long)np * T, heads * 64, c.st), "pag_identity");
            n -= np;
            if (n == 0) return o;
        }
        AttnArgs a;
        a.q = q; a.k = k; a.v = v; a.o = o.p;
        a.ldq = ldq; a.ldk = ldkv; a.ldv = ldkv; a.ldo = o.ld;
        a.sq = sq; a.sk = skv; a.sv = skv; a.so = (long long)T * o.ld;
        a.n = n; a.heads = heads; a.Nq = T; a.Nk = Nk; a.scale = 0.125f;
        c.check(ladi_launch_flash_attn64(a, c.st), "flash_attn64");
        return o;
    }
    // Token merging of one block (runtime.h ToMe): the plan from the block's token input t0 -- prep, match, plan into the block's persistent
    // out_row rows of this forward's samples and into a plan buffer of the arena, which lives until the block releases its mark
    struct Merge { const ToMeLevel* l = nullptr; const int* plan = nullptr; const int* out_row = nullptr; int Tm = 0; };
    Merge tome_plan(const ToMeLevel* l, const Act& t0, int bit) {
        const int n = t0.n, C = t0.c;
        if (C % 64 || C > 960) throw std::runtime_error("token merging: " + std::to_string(C) + " channels (the match kernel takes multiples of 64 up to 960)");
        Merge m; m.l = l; m.Tm = l->T - l->r;
        const long long ps = ladi_tome_plan_ints(l->Ns, l->Nd, l->r);
        int* plan = reinterpret_cast<int*>(c.ar->alloc((size_t)n * ps * sizeof(int)));
        h16* A = c.alloc_h16((size_t)n * ladi_tome_pad_src(l->Ns) * C);
        h16* B = c.alloc_h16((size_t)n * ladi_tome_pad_dst(l->Nd) * C);
        float* score = c.alloc_f32((size_t)n * l->Ns);
        int* node = reinterpret_cast<int*>(c.ar->alloc((size_t)n * l->Ns * sizeof(int)));
        m.plan = plan;
        if (c.dry()) return m;
        int* orow = u.tome.out_row[bit];
        if (!orow) throw std::runtime_error("token merging: block " + std::to_string(bit) + " has no out_row buffer");
        orow += (size_t)sample0 * l->T;
        m.out_row = orow;
        c.check(ladi_launch_tome_prep(t0.p, t0.ld, (long long)l->T * t0.ld, l->src_pos, l->dst_pos, n, l->T, l->Ns, l->Nd, C, A, B, c.st), "tome_prep");
        c.check(ladi_launch_tome_match(A, B, n, l->Ns, l->Nd, C, score, node, c.st), "tome_match");
        c.check(ladi_launch_tome_plan(score, node, l->src_pos, l->dst_pos, n, l->T, l->Ns, l->Nd, l->r, orow, plan, c.st), "tome_plan");
        return m;
    }
    // m(LayerNorm(t)): the LayerNorm the following projection fuses on the plain path is its own launch in front of the merge
    Act tome_merge(const Merge& m, const DNorm& ln, const Act& t) {
        Act a = layer_norm(c, ln, t, 1e-5f);
        Act y = c.new_act(t.n, m.Tm, 1, t.c);
        if (!c.dry())
            c.check(ladi_launch_tome_merge(a.p, a.ld, (long long)m.l->T * a.ld, m.l->dst_pos, m.plan, t.n, m.l->T, m.l->Ns, m.l->Nd, m.l->r, t.c,
                                           y.p, y.ld, (long long)m.Tm * y.ld, c.st), "tome_merge");
        return y;
    }
    // u(y) + res
    Act tome_unmerge(const Merge& m, const Act& y, const Act& res) {
        Act o = c.new_act(res.n, res.h, res.w, res.c);
        if (!c.dry())
            c.check(ladi_launch_tome_unmerge_add(y.p, y.ld, (long long)m.Tm * y.ld, res.p, res.ld, (long long)m.l->T * res.ld, m.out_row, res.n, m.l->T,
                                                 m.Tm, res.c, o.p, o.ld, (long long)m.l->T * o.ld, c.st), "tome_unmerge_add");
        return o;
    }
    // One residual sub-layer of a transformer block over the tokens t [n][T][C]: t + last(core(first(LayerNorm(t)))).  Plain (m null): the
    // LayerNorm is fused into `first` (K = 320 / 640, X-stationary kernel; else its own launch) and the residual into `last`.  Merged:
    // u(last(core(first(m(LayerNorm(t)))))) + t -- the LayerNorm is its own launch in front of the merge and the unmerge kernel adds the residual.
    // core(a, rows) maps the projected tokens a [n][rows][.] to the input of `last`; rows is T, or T - r when merged
    template <typename Core>
    Act sublayer(const Merge* m, const DNorm& ln, const DConv& first, ConvOpt of, const DConv& last, const Act& t, int T, Core&& core) {
        Act a;
        if (m) a = conv2d(c, first, tome_merge(*m, ln, t), nullptr, of);
        else { of.ln = &ln; a = conv2d(c, first, t, nullptr, of); }
        Act y = core(a, m ? m->Tm : T);
        ConvOpt ol; if (!m) ol.res0 = &t;
        Act o = conv2d(c, last, y, nullptr, ol);
        return m ? tome_unmerge(*m, o, t) : o;
    }
    Act xf(const XfBlock& b, const Act& x) {
        const int n = x.n, T = x.h * x.w, C = b.C, bit = b.bit, level = b.level;
        int np = 0;
        if (pag_first != PAG_NONE && ((u.pag_mask >> bit) & 1u)) {
            const int lead = pag_first - sample0;                       // leading unperturbed samples of this forward
            np = n - (lead < 0 ? 0 : lead > n ? n : lead);
        }
        const ToMeLevel* tl = nullptr;
        if (u.tome.on && level < u.tome.cfg.max_downsample) {
            // a planning pass sizes the buffers for the whole context batch at once (the lanes and the sub-batch forms plan one after the other)
            const int need = c.dry() && u.ctx_n > sample0 + n ? u.ctx_n : sample0 + n;
            tl = u.tome_prepare(level, x.h, x.w, need, c.dry());
            if (tl->r == 0) tl = nullptr;
            else if (np > 0) throw std::runtime_error("UNet::forward: perturbed samples in a transformer block that merges tokens");
        }
        const ToMeCfg& tc = u.tome.cfg;
        const bool m1 = tl && tc.merge_attn, m2 = tl && tc.merge_crossattn, m3 = tl && tc.merge_mlp;
        Act out = new_act_with_stats(c, x.n, x.h, x.w, C);
        const size_t mk = c.ar->mark();
        // GroupNorm (no activation) -> proj_in: the normalisation's affine is applied to proj_in's register panel where the X-stationary
        // kernel carries the projection (64x48 / 32x24 levels), else as its own pass
        ConvOpt op;
        Act tok;
        if (gn_fusable(x, b.proj_in.cout)) {
            op.gn_ss = gn_scale_shift(c, b.gn, x, nullptr, u.cfg.groups, 1e-6f);
            tok = x;
        } else tok = group_norm(c, b.gn, x, nullptr, u.cfg.groups, 1e-6f, 0);
        tok.h = T; tok.w = 1;  // tokens view [n][T][C]
        tok.st_part = nullptr; tok.st_px = 0;
        Act t0 = conv2d(c, b.proj_in, tok, nullptr, op);
        // token merging: one plan per block from t0; a merged sub-layer is u(f(m(LayerNorm(t)))) + t, its output projection without the fused
        // residual, which the unmerge kernel adds
        Merge mg;
        if (tl) mg = tome_plan(tl, t0, bit);
        // SAG map of the mid block: the column sums of attn1's softmax, from the Q and K the attention is about to read, into the rows of
        // this forward's samples; the scratch of the two-stage sum lives in the arena until the block releases its mark
        const bool sag_here = sag && bit == u.mid_bit;
        if (sag_here) {
            if (m1) throw std::runtime_error("UNet::forward: the SAG map in a transformer block that merges tokens");
            const int need = c.dry() && u.ctx_n > sample0 + n ? u.ctx_n : sample0 + n;
            u.sag_prepare(T, need, c.dry());
        }
        Act t1 = sublayer(m1 ? &mg : nullptr, b.ln1, b.qkv, ConvOpt(), b.o1, t0, T, [&](const Act& qkv, int T1) {
            if (sag_here) {
                float* part = c.alloc_f32((size_t)ladi_sag_partial_floats(n, T1, b.heads));
                if (!c.dry())
                    c.check(ladi_launch_sag_map(qkv.p, 3 * C, (long long)T1 * 3 * C, qkv.p + C, 3 * C, (long long)T1 * 3 * C, n, T1, b.heads, part,
                                                u.sag_s + (size_t)sample0 * T1, u.sag_m + (size_t)sample0 * T1, c.st), "sag_map");
            }
            return attn(qkv.p, 3 * C, (long long)T1 * 3 * C, qkv.p + C, qkv.p + 2 * C, 3 * C, (long long)T1 * 3 * C, n, T1, T1, b.heads, np);
        });
        // attn2 and the feed-forward as ONE kernel each on the C = 320 level (xf_fused.hip; LADI_XF_FUSE=0 / =1 / =2: none / attn2 only / both,
        // latched at UNet::load), else the chain of projections.  Measured on
        // MI355X (profiles/r05_xf_fused_ab.txt): parity-green and bit-reproducible, but at one wave per SIMD the fused chains expose the latency two
        // waves per SIMD hide in the separate launches -- attn2 85.7 us against the ~76 us of the three launches it replaces (forward
        // +0.05 ms), feed-forward 275 us against 109 + 57 us (forward +0.45 ms) -- so the DEFAULT IS OFF; the kernels stay selectable.
        // an image context (IP-Adapter) with a non-zero scale for this block: the chain of projections, with the image term accumulated into
        // the attention output before to_out
        const bool ip = u.ip_ctx_n > 0 && b.ip_scale != 0.f;
        int fuse = 0;
        if (!ip && b.o2_packed && b.kp_tiles && t1.ld == C && ladi_xf_fused_eligible(C, b.heads, T, u.ctx_L)) fuse = u.xf_fuse;
        Act t2;
        if (fuse >= 1 && !m2) {                      // a sub-layer that merges runs the chain of projections
            t2 = c.new_act(n, T, 1, C);
            if (!c.dry()) {
                XAttnBlockArgs xa;
                xa.x = t1.p; xa.ln_g = b.ln2.g; xa.ln_b = b.ln2.b; xa.ln_eps = 1e-5f;
                xa.Wq = b.q2.w;
                xa.Kp = b.kp_tiles + ladi_xf_kp_elems(sample0); xa.Vt = b.vt_tiles + ladi_xf_vt_elems(sample0);
                xa.Wo = b.o2_packed; xa.bo = b.o2.b; xa.res = t1.p; xa.out = t2.p;
                xa.P = n * T; xa.T = T; xa.nk = u.ctx_L; xa.scale = 0.125f;
                c.check(ladi_launch_xattn_block(xa, c.st), "xattn_block");
            }
        } else {
            // merged: the queries (and the image term's) are the T - r merged rows
            t2 = sublayer(m2 ? &mg : nullptr, b.ln2, b.q2, ConvOpt(), b.o2, t1, T, [&](const Act& q2, int T2) {
                const h16* kv = b.kv_cache + (size_t)sample0 * u.ctx_L * 2 * C;     // this lane's samples of the cached cross-attention K / V
                Act o2 = attn(q2.p, C, (long long)T2 * C, kv, kv + C, 2 * C, (long long)u.ctx_L * 2 * C, n, T2, u.ctx_L, b.heads);
                if (!ip) return o2;
                const long long skv = (long long)u.ip_ctx_N * 2 * C;
                const h16* ikv = b.ip_kv_cache + (size_t)sample0 * skv;           // this lane's samples of the image K / V
                if (u.ip_route == 1) {
                    Act oi = attn(q2.p, C, (long long)T2 * C, ikv, ikv + C, 2 * C, skv, n, T2, u.ip_ctx_N, b.heads);
                    if (!c.dry()) c.check(ladi_launch_ip_scaled_add(oi.p, oi.ld, o2.p, o2.ld, (long long)n * T2, C, b.ip_scale, c.st), "ip_scaled_add");
                } else if (!c.dry()) {
                    c.check(ladi_launch_ip_attn_add(q2.p, q2.ld, (long long)T2 * q2.ld, ikv, 2 * C, skv, ikv + C, 2 * C, skv, o2.p, o2.ld, (long long)T2 * o2.ld,
                                                    n, b.heads, T2, u.ip_ctx_N, b.ip_scale, c.st), "ip_attn_add");
                }
                return o2;
            });
        }
        Act t3;
        if (fuse >= 2 && !m3) {
            t3 = c.new_act(n, T, 1, C);
            if (!c.dry()) {
                FFBlockArgs fa;
                fa.x = t2.p; fa.ln_g = b.ln3.g; fa.ln_b = b.ln3.b; fa.ln_eps = 1e-5f;
                fa.W1 = b.ff1.w; fa.b1 = b.ff1.b; fa.W2 = b.ff2_packed; fa.bo = b.ff2.b; fa.res = t2.p; fa.out = t3.p; fa.P = n * T;
                c.check(ladi_launch_ff_block(fa, c.st), "ff_block");
            }
        } else {
            ConvOpt og; og.act = LADI_ACT_GEGLU;
            t3 = sublayer(m3 ? &mg : nullptr, b.ln3, b.ff1, og, b.ff2, t2, T, [](const Act& gg, int) { return gg; });
        }
        Act xin = x; xin.h = T; xin.w = 1;
        Act outv = out; outv.h = T; outv.w = 1;
        ConvOpt oo; oo.res0 = &xin; oo.dst = &outv;
        (void)conv2d(c, b.proj_out, t3, nullptr, oo);
        out.st_part = outv.st_part; out.st_px = outv.st_px;
        c.ar->release(mk);
        return out;
    }
};

}  // namespace

Act UNet::forward(Ctx& c, const Act& x, const float* temb_row, const int* temb_idx, const FwdOpt& opt) {
    const Act* eps_out = opt.eps_out; const FeatCache* fc = opt.fc;
    const int sample0 = opt.sample0, pag_first = opt.pag_first;
    // deep-feature cache (runtime.h FeatCache): `shallow` skips every layer outside the 64x48 level's outermost `branch` layers; the layer
    // sequence below stays the only one -- a skipped layer only advances the weight indices
    const int L = cfg.layers_per_block;
    const int fmode = fc ? fc->mode : FeatCache::NONE, fbranch = fc ? fc->branch : 0;
    const bool shallow = fmode == FeatCache::SHALLOW;
    if (fmode != FeatCache::NONE && (fbranch < 0 || fbranch > L || (!fc->buf && !c.dry())))
        throw std::runtime_error("UNet::forward: feature cache needs a buffer and a branch in [0, layers_per_block]");
    // the cached tensor: rows of this forward's samples, [n, h, w, fc_channels(branch)] dense, no producer statistics
    auto cache_view = [&]() {
        Act a; a.n = x.n; a.h = x.h; a.w = x.w; a.c = fc_channels(fbranch); a.ld = a.c;
        a.p = fc->buf ? fc->buf + (size_t)sample0 * x.h * x.w * a.c : nullptr;
        return a;
    };
    if ((eps_out ? sample0 + x.n > ctx_n : ctx_n != x.n) && !c.dry()) throw std::runtime_error("UNet::forward: set_context batch mismatch");
    if (ip_ctx_n > 0 && ip_ctx_n != ctx_n && !c.dry())
        throw std::runtime_error("UNet::forward: image context batch mismatch: " + std::to_string(ip_ctx_n) + " samples, set_context has " + std::to_string(ctx_n));
    if (pag_first != PAG_NONE && fmode != FeatCache::NONE) throw std::runtime_error("UNet::forward: perturbed samples together with a feature cache");
    Fwd f{c, *this, temb_row, temb_idx, sample0, pag_first, opt.sag < 0 ? sag_capture : opt.sag != 0};
    ProbeScope probe_scope(c, probe);
    // range probe points, named by the diffusers key prefix of the module that produced the tensor (off: one pointer test each)
    auto pp = [&](const Act& a, const char* fmt, int i = 0, int j = 0) {
        if (!c.probe) return;
        char name[64];
        std::snprintf(name, sizeof(name), fmt, i, j);
        c.probe_point(name, a);
    };
    std::vector<Act> skips;
    ConvOpt o; o.stats = true;
    Act h = conv2d(c, conv_in, x, nullptr, o);
    pp(h, "conv_in");
    skips.push_back(h);
    int ri = 0, xi = 0;     // xi walks UNet::xf once, down to up: every transformer block, run or skipped, advances it
    for (int i = 0; i < 4; ++i) {
        for (int j = 0; j < L; ++j) {
            if (shallow && (i > 0 || j >= fbranch)) { ++ri; if (i < 3) ++xi; continue; }
            h = f.res(down_res[ri++], h, nullptr);
            pp(h, "down_blocks.%d.resnets.%d", i, j);
            if (i < 3) { h = f.xf(xf[xi++], h); pp(h, "down_blocks.%d.attentions.%d", i, j); }
            skips.push_back(h);
        }
        if (i < 3 && !shallow) {
            ConvOpt od; od.stride = 2; od.pad = 1; od.stats = true;
            h = conv2d(c, down_samp[i], h, nullptr, od);
            pp(h, "down_blocks.%d.downsamplers.0", i);
            skips.push_back(h);
        }
    }
    if (!shallow) {
        h = f.res(mid_res[0], h, nullptr);
        pp(h, "mid_block.resnets.0");
        h = f.xf(xf[xi], h);
        pp(h, "mid_block.attentions.0");
        h = f.res(mid_res[1], h, nullptr);
        pp(h, "mid_block.resnets.1");
    }
    ++xi;
    // diffusers' `forward_upsample_size`: when a latent side is not a multiple of 2^3 (three upsamplers), the down path rounded a level up
    // (ceil(H / 2)) and every upsampler stretches to the size of the skip it is concatenated with; else each one doubles
    const bool ups_to_skip = (x.h % 8) || (x.w % 8);
    ri = 0;
    for (int i = 0; i < 4; ++i) {
        for (int j = 0; j < L + 1; ++j) {
            // the cache point: the hidden state that enters up_blocks.3.resnets.(L - branch), before the concatenation with its skip
            const bool cache_pt = fmode != FeatCache::NONE && i == 3 && j == L - fbranch;
            if (shallow && !cache_pt && (i < 3 || j < L - fbranch)) { ++ri; if (i > 0) ++xi; continue; }
            if (cache_pt) {
                Act cv = cache_view();
                if (shallow) h = cv;
                else {
                    if (h.n != cv.n || h.h != cv.h || h.w != cv.w || h.c != cv.c || h.ld != h.c)
                        throw std::runtime_error("UNet::forward: the tensor at the cache point does not have the cache's shape");
                    if (!c.dry()) {
                        hipError_t e = hipMemcpyAsync(cv.p, h.p, h.pixels() * (size_t)h.c * sizeof(h16), hipMemcpyDeviceToDevice, c.st);
                        if (e != hipSuccess) throw std::runtime_error(std::string("UNet::forward: feature cache capture: ") + hipGetErrorString(e));
                    }
                }
            }
            Act sk = skips.back(); skips.pop_back();
            if (freeu.on && i < 2) {
                // FreeU site (runtime.h FreeU): in place, nothing is allocated.  The producers' statistics rows describe the unmodified
                // tensors: the consuming GroupNorm computes them from the data, as it does for the cached tensor
                if (!c.dry())
                    c.check(ladi_launch_freeu(h.p, h.ld, h.c, i ? freeu.b2 : freeu.b1, sk.p, sk.ld, sk.c, i ? freeu.s2 : freeu.s1, sk.p, sk.ld,
                                              h.n, h.h, h.w, c.st), "freeu");
                h.st_part = nullptr; h.st_px = 0;
                sk.st_part = nullptr; sk.st_px = 0;
            }
            h = f.res(up_res[ri++], h, &sk);
            pp(h, "up_blocks.%d.resnets.%d", i, j);
            if (i > 0) { h = f.xf(xf[xi++], h); pp(h, "up_blocks.%d.attentions.%d", i, j); }
        }
        if (i < 3 && !shallow) {
            ConvOpt ou; ou.ups = 1; ou.stats = true;
            if (ups_to_skip) { ou.ups_h = skips.back().h; ou.ups_w = skips.back().w; }
            h = conv2d(c, up_samp[i], h, nullptr, ou);
            pp(h, "up_blocks.%d.upsamplers.0", i);
        }
    }
    Act g = group_norm(c, norm_out, h, nullptr, cfg.groups, cfg.eps, 1);
    ConvOpt oc; oc.out_ld = 4;
    if (cfg.out_channels > 4) oc.out_ld = (cfg.out_channels + 3) / 4 * 4;
    Act eps;
    if (eps_out) { eps = *eps_out; oc.dst = &eps; }     // a sample-group lane writes its rows of the shared output
    Act out = conv2d(c, conv_out, g, nullptr, oc);
    pp(out, "conv_out");
    return out;
}

void UNet::key(Key& k, bool perturbed, int sag) const {
    if (xf.empty()) throw std::runtime_error("UNet::key: the UNet is not loaded");
    k.temb_table = temb_table; k.kv_cache = xf.front().kv_cache;
    k.probe = probe ? probe->id : 0ULL;
    if (freeu.on) {
        const float fv[4] = {freeu.s1, freeu.s2, freeu.b1, freeu.b2};
        k.freeu_on = 1; std::memcpy(k.freeu, fv, sizeof(fv));
    }
    if (perturbed) k.pag_mask = pag_mask;
    if (ip_ctx_n > 0) {
        k.ip_on = 1; k.ip_N = ip_ctx_N; k.ip_kv = xf.front().ip_kv_cache;
        for (auto& b : xf) if (b.bit < 32) std::memcpy(&k.ip_scale[b.bit], &b.ip_scale, 4);
    }
    if (tome.on) {
        const ToMeCfg& tc = tome.cfg;
        const int opts[8] = {tc.max_downsample, tc.sx, tc.sy, tc.use_rand, (int)tc.seed, tc.merge_attn, tc.merge_crossattn, tc.merge_mlp};
        k.tome_on = 1; std::memcpy(k.tome_opts, opts, sizeof(opts));
        std::memcpy(&k.tome_ratio, &tc.ratio, sizeof(double)); k.tome_gen = tome.gen;
    }
    if (sag < 0 ? sag_capture : sag != 0) { k.sag_on = 1; k.sag_buf = sag_mem; }
}

// ------------------------------------------------------------------------------------------------
// Sample-group lanes (runtime.h): G forwards of n / G samples on G streams
// ------------------------------------------------------------------------------------------------
#define HIP_OK_L(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) throw std::runtime_error(std::string(#x) + ": " + hipGetErrorString(e_)); } while (0)

int UNetLanes::pick(int n) {
    int want = 1;
    if (const char* e = getenv("LADI_UNET_LANES")) want = atoi(e);
    if (want < 1) want = 1;
    if (want > MAXG) want = MAXG;
    while (want > 1 && (n % want)) --want;
    return want;
}

void UNetLanes::reset() {
    for (int i = 0; i < MAXG; ++i) {
        if (st[i]) (void)hipStreamSynchronize(st[i]);
        arena[i].~Arena(); new (&arena[i]) Arena();
        peak[i] = 0; stats_peak[i] = 0;
    }
}

void UNetLanes::configure(int n, int g) {
    const int want = g > 0 ? g : pick(n);
    if (want != G && arena[0].cap) reset();     // another lane count than the one the arenas were planned for: start from a clean plan
    G = want;
    if (G < 1 || G > MAXG || (n % G)) throw std::runtime_error("UNetLanes: the lane count must divide the sample count");
    if (!fork) HIP_OK_L(hipEventCreateWithFlags(&fork, hipEventDisableTiming));
    for (int i = 1; i < G; ++i) {
        if (!st[i]) HIP_OK_L(hipStreamCreateWithFlags(&st[i], hipStreamNonBlocking));
        if (!join[i]) HIP_OK_L(hipEventCreateWithFlags(&join[i], hipEventDisableTiming));
    }
}

void UNetLanes::forward(UNet& u, hipStream_t main_st, bool dry, bool concurrent, const Act& x, const Act& eps, const float* temb, const int* tidx,
                        const FwdOpt& o) {
    const int Gu = sub_lanes(x.n);          // the configured count when it divides x.n (always, for the whole batch)
    const int ng = x.n / Gu;
    const bool par = concurrent && !dry && Gu > 1;
    if (par) HIP_OK_L(hipEventRecord(fork, main_st));
    for (int g = 0; g < Gu; ++g) {
        hipStream_t sg = (par && g > 0) ? st[g] : main_st;
        if (par && g > 0) HIP_OK_L(hipStreamWaitEvent(sg, fork, 0));
        arena[g].dry = dry; arena[g].off = 0;
        Ctx c; c.st = sg; c.ar = &arena[g]; c.stats = stats[g]; c.stats_cap = stats_cap[g]; c.sk_cnt = sk_cnt[g];
        if (!dry && stats_cap[g]) HIP_OK_L(hipMemsetAsync(stats[g], 0, stats_cap[g] * sizeof(float), sg));
        Act xg = x; xg.n = ng; xg.p = x.p + (size_t)g * ng * x.h * x.w * x.ld;
        Act eg = eps; eg.n = ng; eg.p = eps.p + (size_t)g * ng * eps.h * eps.w * eps.ld; eg.st_part = nullptr; eg.st_px = 0;
        FwdOpt og = o; og.eps_out = &eg; og.sample0 = o.sample0 + g * ng;
        (void)u.forward(c, xg, temb, tidx, og);
        if (dry) { peak[g] = arena[g].peak; if (c.stats_peak > stats_peak[g]) stats_peak[g] = c.stats_peak; }
        if (par && g > 0) { HIP_OK_L(hipEventRecord(join[g], sg)); HIP_OK_L(hipStreamWaitEvent(main_st, join[g], 0)); }
    }
}

void UNetLanes::commit_plan() {
    for (int g = 0; g < G; ++g) {
        if (!sk_cnt[g]) {
            HIP_OK_L(hipMalloc(reinterpret_cast<void**>(&sk_cnt[g]), 1024 * sizeof(int)));
            HIP_OK_L(hipMemset(sk_cnt[g], 0, 1024 * sizeof(int)));
        }
        arena[g].reserve(peak[g] + 4096);
        if (stats_peak[g] > stats_cap[g]) {
            if (stats[g]) (void)hipFree(stats[g]);
            stats[g] = nullptr;
            HIP_OK_L(hipMalloc(reinterpret_cast<void**>(&stats[g]), stats_peak[g] * sizeof(float)));
            stats_cap[g] = stats_peak[g];
        }
    }
}

void UNetLanes::key(Key& k) const {
    k.G = G;
    for (int g = 0; g < MAXG; ++g) {
        k.arena[g] = g < G ? arena[g].base : nullptr;
        k.stats[g] = g < G ? stats[g] : nullptr;
    }
}

UNetLanes::~UNetLanes() {
    for (int i = 0; i < MAXG; ++i) {
        if (stats[i]) (void)hipFree(stats[i]);
        if (sk_cnt[i]) (void)hipFree(sk_cnt[i]);
        if (join[i]) (void)hipEventDestroy(join[i]);
        if (st[i]) (void)hipStreamDestroy(st[i]);
    }
    if (fork) (void)hipEventDestroy(fork);
}

}  // namespace ladi
