// extern "C" boundary of libladi_native (see include/ladi_native.h for the contract and reference citations).
#include "../../include/ladi_native.h"
#include "runtime.h"
#include <mutex>
#include <stdexcept>
#include <vector>
#include <cstring>
#include <cmath>
#include <algorithm>

using namespace ladi;

#define HIP_OK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) throw std::runtime_error(std::string(#x) + ": " + hipGetErrorString(e_)); } while (0)

struct ladi_weights { WeightStore ws; };
struct ladi_unet { UNet u; UNetLanes lanes; Arena io; };
struct ladi_vae { VAE v; };
struct ladi_emasc { EMASC e; };
struct ladi_adapter { Adapter a; };
struct ladi_text_encoder { TextEncoder t; };
struct ladi_vision_encoder { VisionEncoder v; };
struct ladi_resampler { Resampler r; };
struct ladi_refine { Refine r; };
struct ladi_tps { Tps t; };
struct ladi_tryon { TryOn t; };
struct ladi_probe { Probe p; explicit ladi_probe(int n) : p(n) {} };
// how many modules point at each probe: ladi_probe_destroy refuses while the count is not zero; attaching, detaching and destroying a module
// keep it (set_module_probe)
static std::mutex g_probe_mu;
static std::unordered_map<const Probe*, int> g_probe_refs;
static void set_module_probe(Probe*& slot, ladi_probe* p) {
    std::lock_guard<std::mutex> lk(g_probe_mu);
    if (slot) --g_probe_refs[slot];
    slot = p ? &p->p : nullptr;
    if (slot) ++g_probe_refs[slot];
}
static_assert(TRYON_CALLBACK_ABORT == LADI_TRYON_CALLBACK_ABORTED, "callback abort code");
static_assert(TRYON_IP_NO_ADAPTER == LADI_TRYON_IP_NO_ADAPTER, "IP-Adapter refusal code");
static_assert(TRYON_IP_ADAPTER_KIND == LADI_TRYON_IP_ADAPTER_KIND, "IP-Adapter kind refusal code");

static_assert(sizeof(ladi_igemm_desc) == sizeof(IGemmArgs), "public igemm descriptor must mirror IGemmArgs");
static_assert(sizeof(ladi_conv_f32_desc) == sizeof(ConvF32Args), "public fp32 convolution descriptor must mirror ConvF32Args");

static inline hipStream_t S(void* s) { return reinterpret_cast<hipStream_t>(s); }

template <typename F>
static int guarded(const char* where, F&& f) {
    try { return f(); }
    catch (const std::exception& e) { set_error(std::string(where) + ": " + e.what()); return -100; }
    catch (...) { set_error(std::string(where) + ": unknown exception"); return -101; }
}

static void require_gpu() {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) throw std::runtime_error("no HIP device: libladi_native has no CPU fallback");
}

namespace {
// Arena of the op-level GroupNorm: one grow-only arena per (device, stream), never freed while the process lives, so a steady-state call
// neither allocates nor synchronises (growing goes through Arena::reserve, whose hipFree waits for the work still reading the old buffer).
// Calls are serialised: the planning state of an arena is not shareable.
struct OpArena { int dev; hipStream_t st; Arena* ar; };
std::mutex g_op_mu;
Arena& op_arena(hipStream_t st) {
    static std::vector<OpArena> pool;
    int dev = 0;
    HIP_OK(hipGetDevice(&dev));
    for (auto& e : pool)
        if (e.dev == dev && e.st == st) return *e.ar;
    pool.push_back(OpArena{dev, st, new Arena()});
    return *pool.back().ar;
}
Act op_view(const void* p, int n, int HW, int C) {
    Act a; a.p = reinterpret_cast<h16*>(const_cast<void*>(p)); a.n = n; a.h = HW; a.w = 1; a.c = C; a.ld = C;
    return a;
}
}  // namespace

// The body of the stand-alone forward entries (ladi_unet_forward, _forward_pag, _forward_cached_rows): null pointers are refused, then
// `checks` -- the entry's own refusals and preparation, by throwing --, the time embedding, and in the UNet's own arena NCHW -> NHWC,
// UNet::forward into an output view, NHWC -> NCHW; `done` is the entry's own bookkeeping after everything was queued
template <typename Checks, typename Done>
static int unet_forward_entry(const char* where, ladi_unet* u, const void* sample, int dtype, int n, int h, int w, float timestep, void* out,
                              int out_dtype, FwdOpt o, void* stream, Checks&& checks, Done&& done) {
    return guarded(where, [&]() {
        if (!u) throw std::runtime_error("null handle");
        if (!sample || !out) throw std::runtime_error("null argument");
        UNet& U = u->u;
        hipStream_t st = S(stream);
        checks(U);
        if (U.compute_temb(&timestep, 1, st)) return -1;
        const int eps_ld = (U.cfg.out_channels + 3) / 4 * 4;
        run_planned(U.arena, st, [&](Ctx& c) {
            Act x = c.new_act(n, h, w, 64);
            Act eo = c.new_act(n, h, w, U.cfg.out_channels, eps_ld);
            o.eps_out = &eo;
            if (!c.dry()) c.check(ladi_launch_nchw_to_nhwc(sample, dtype == LADI_F32, n, U.cfg.in_channels, h, w, x.p, 64, st), "nchw_to_nhwc");
            Act eps = U.forward(c, x, U.temb_table, nullptr, o);
            if (!c.dry()) c.check(ladi_launch_nhwc_to_nchw(eps.p, eps.ld, n, U.cfg.out_channels, h, w, out, out_dtype == LADI_F32, st), "nhwc_to_nchw");
        }, &U.stats, &U.stats_cap);
        done(U);
        return 0;
    });
}

extern "C" {

const char* ladi_last_error(void) { return last_error(); }
int ladi_version(void) { return 100; }
int ladi_device_count(void) { int n = 0; if (hipGetDeviceCount(&n) != hipSuccess) return 0; return n; }

// ------------------------------------------------------------------------------------------------ weights
ladi_weights* ladi_weights_create(void) { return new (std::nothrow) ladi_weights(); }
int ladi_weights_add(ladi_weights* w, const char* key, const void* data, int dtype, int ndim, const int64_t* shape) {
    return guarded("ladi_weights_add", [&]() {
        if (!w || !key || !data || ndim < 0 || ndim > 8) throw std::runtime_error("bad arguments");
        HostTensor t;
        t.shape.assign(shape, shape + ndim);
        const size_t n = t.numel();
        t.data.resize(n);
        if (dtype == LADI_F32) std::memcpy(t.data.data(), data, n * 4);
        else if (dtype == LADI_F16) { const _Float16* h = reinterpret_cast<const _Float16*>(data); for (size_t i = 0; i < n; ++i) t.data[i] = (float)h[i]; }
        else throw std::runtime_error("unsupported dtype");
        w->ws.m[key] = std::move(t);
        return 0;
    });
}
int ladi_weights_count(const ladi_weights* w) { return w ? (int)w->ws.m.size() : -1; }
void ladi_weights_destroy(ladi_weights* w) { delete w; }

// ------------------------------------------------------------------------------------------------ UNet
ladi_unet* ladi_unet_create(const ladi_unet_config* cfg, const ladi_weights* ws) {
    ladi_unet* h = nullptr;
    int rc = guarded("ladi_unet_create", [&]() {
        if (!cfg || !ws) throw std::runtime_error("null argument");
        require_gpu();
        UNetCfg c;
        c.in_channels = cfg->in_channels; c.out_channels = cfg->out_channels;
        for (int i = 0; i < 4; ++i) { c.boc[i] = cfg->block_out_channels[i]; c.heads[i] = cfg->num_heads[i]; }
        c.layers_per_block = cfg->layers_per_block; c.cross_dim = cfg->cross_attention_dim; c.groups = cfg->norm_num_groups; c.eps = cfg->norm_eps;
        if (c.in_channels > 64) throw std::runtime_error("in_channels > 64 unsupported");
        h = new ladi_unet();
        h->u.load(c, ws->ws);
        return 0;
    });
    if (rc) { delete h; return nullptr; }
    return h;
}
void ladi_unet_destroy(ladi_unet* u) { if (u) set_module_probe(u->u.probe, nullptr); delete u; }

int ladi_unet_set_context(ladi_unet* u, const void* ehs, int n, int L, void* stream) {
    return guarded("ladi_unet_set_context", [&]() { return u->u.set_context(reinterpret_cast<const h16*>(ehs), n, L, S(stream)); });
}

int ladi_unet_set_freeu(ladi_unet* u, int on, float s1, float s2, float b1, float b2) {
    if (!u) { set_error("ladi_unet_set_freeu: null handle"); return -1; }
    FreeU f;
    if (on) {
        if (!std::isfinite(s1) || !std::isfinite(s2) || !std::isfinite(b1) || !std::isfinite(b2)) {
            set_error("ladi_unet_set_freeu: s1, s2, b1 and b2 have to be finite");
            return -1;
        }
        f.on = true; f.s1 = s1; f.s2 = s2; f.b1 = b1; f.b2 = b2;
    }
    u->u.freeu = f;
    return 0;
}

int ladi_unet_pag_layer_count(const ladi_unet* u) { return u ? u->u.pag_layer_count() : -1; }
int ladi_unet_set_pag_layers(ladi_unet* u, unsigned layer_mask) {
    if (!u) { set_error("ladi_unet_set_pag_layers: null handle"); return -1; }
    const int cnt = u->u.pag_layer_count();
    if (layer_mask == 0 || (cnt < 32 && (layer_mask >> cnt))) {
        set_error("ladi_unet_set_pag_layers: the mask " + std::to_string(layer_mask) + " selects no transformer block or has bits beyond the " +
                  std::to_string(cnt) + " blocks of this UNet");
        return -1;
    }
    u->u.pag_mask = layer_mask;
    return 0;
}
unsigned ladi_unet_pag_layers(const ladi_unet* u) { return u ? u->u.pag_mask : 0u; }
int ladi_unet_set_sag_capture(ladi_unet* u, int on) {
    if (!u) { set_error("ladi_unet_set_sag_capture: null handle"); return -1; }
    u->u.sag_capture = on != 0;
    return 0;
}
int ladi_unet_sag_tokens(const ladi_unet* u, int h, int w, int* hm, int* wm) {
    if (!u || !hm || !wm || h < 1 || w < 1) { set_error("ladi_unet_sag_tokens: null argument or an empty latent size"); return -1; }
    UNet::sag_tokens(h, w, hm, wm);
    return 0;
}
int ladi_unet_sag_map(ladi_unet* u, float* s_out, unsigned char* m_out, int n, int T) {
    return guarded("ladi_unet_sag_map", [&]() {
        if (!u || (!s_out && !m_out)) throw std::runtime_error("null handle or no output");
        const UNet& U = u->u;
        if (!U.sag_mem || U.sag_T < 1) throw std::runtime_error("no forward has captured a SAG map (ladi_unet_set_sag_capture, or a SAG run)");
        if (T != U.sag_T || n < 1 || n > U.sag_cap_n)
            throw std::runtime_error("asked for " + std::to_string(n) + " samples of " + std::to_string(T) + " tokens, the last capture has " +
                                     std::to_string(U.sag_T) + " tokens and room for " + std::to_string(U.sag_cap_n) + " samples");
        HIP_OK(hipDeviceSynchronize());
        if (s_out) HIP_OK(hipMemcpy(s_out, U.sag_s, (size_t)n * T * sizeof(float), hipMemcpyDeviceToDevice));
        if (m_out) HIP_OK(hipMemcpy(m_out, U.sag_m, (size_t)n * T, hipMemcpyDeviceToDevice));
        return 0;
    });
}

// ------------------------------------------------------------------------------------------------ token merging (runtime.h ToMe, tome.hip)
static ToMeCfg tome_from(const ladi_tome_config& c) {
    ToMeCfg t;
    t.ratio = c.ratio; t.max_downsample = c.max_downsample; t.sx = c.sx; t.sy = c.sy; t.use_rand = c.use_rand; t.seed = c.seed;
    t.merge_attn = c.merge_attn; t.merge_crossattn = c.merge_crossattn; t.merge_mlp = c.merge_mlp;
    return t;
}
int ladi_tome_config_check(const ladi_tome_config* cfg) {
    if (!cfg) { set_error("ladi_tome_config_check: null configuration"); return -1; }
    const std::string e = tome_cfg_error(tome_from(*cfg));
    if (!e.empty()) { set_error("ladi_tome_config_check: " + e); return -1; }
    return 0;
}
int ladi_unet_set_token_merging(ladi_unet* u, const ladi_tome_config* cfg) {
    if (!u) { set_error("ladi_unet_set_token_merging: null handle"); return -1; }
    try {
        if (cfg) { const ToMeCfg t = tome_from(*cfg); u->u.tome_set(&t); }
        else u->u.tome_set(nullptr);
    } catch (const std::exception& e) { set_error(std::string("ladi_unet_set_token_merging: ") + e.what()); return -1; }
    return 0;
}
int ladi_unet_token_merging(const ladi_unet* u, ladi_tome_config* cfg_out) {
    if (!u) { set_error("ladi_unet_token_merging: null handle"); return -1; }
    if (cfg_out) {
        const ToMeCfg& t = u->u.tome.cfg;
        cfg_out->ratio = t.ratio; cfg_out->max_downsample = t.max_downsample; cfg_out->sx = t.sx; cfg_out->sy = t.sy; cfg_out->use_rand = t.use_rand;
        cfg_out->seed = t.seed; cfg_out->merge_attn = t.merge_attn; cfg_out->merge_crossattn = t.merge_crossattn; cfg_out->merge_mlp = t.merge_mlp;
    }
    return u->u.tome.on ? 1 : 0;
}
int ladi_unet_tome_block_count(const ladi_unet* u, int* blocks_out, int cap) {
    if (!u) { set_error("ladi_unet_tome_block_count: null handle"); return -1; }
    const std::vector<int> b = u->u.tome_blocks();
    for (int i = 0; blocks_out && i < (int)b.size() && i < cap; ++i) blocks_out[i] = b[i];
    return (int)b.size();
}
int ladi_unet_tome_read_plan(ladi_unet* u, int block, int* out_row_host, int cap) {
    return guarded("ladi_unet_tome_read_plan", [&]() {
        if (!u) throw std::runtime_error("null handle");
        const std::vector<int> b = u->u.tome_blocks();
        if (block < 0 || block >= (int)b.size()) throw std::runtime_error("block " + std::to_string(block) + " is outside the " + std::to_string(b.size()) + " merged blocks");
        const ToMeLevel& l = u->u.tome.lv[u->u.xf[b[block]].level];
        const int* src = u->u.tome.out_row[b[block]];
        if (!src || l.r == 0) return 0;
        const int n = u->u.ctx_n < l.cap_n ? u->u.ctx_n : l.cap_n;
        const long long cnt = (long long)n * l.T;
        if (cnt > 0x7fffffffLL) throw std::runtime_error("the plan has more than 2^31 entries");
        if (out_row_host && cap >= cnt && cnt > 0) {
            HIP_OK(hipDeviceSynchronize());
            HIP_OK(hipMemcpy(out_row_host, src, (size_t)cnt * sizeof(int), hipMemcpyDeviceToHost));
        }
        return (int)cnt;
    });
}
int ladi_tome_tables(int h, int w, int sx, int sy, int use_rand, unsigned seed, int* src_pos, int* dst_pos, int cap) {
    const int rc = ladi_tome_tables_host(h, w, sx, sy, use_rand, seed, src_pos, dst_pos, cap);
    if (rc < 0) set_error("ladi_tome_tables: refused: h or w < 1, sx or sy other than 2, one table pointer without the other, or cap below max(Nd, h w - Nd)");
    return rc;
}
int ladi_tome_merge_count(int T, int Ns, double ratio) {
    const int rc = ladi_tome_count_host(T, Ns, ratio);
    if (rc < 0) set_error("ladi_tome_merge_count: T < 1, Ns < 0 or a ratio outside [0, 1)");
    return rc;
}
static int tome_op_rc(const char* what, int rc) {
    if (rc == -1) set_error(std::string(what) + ": refused: a null pointer or a bad count (n, T, Ns + Nd != T, r)");
    else if (rc == -2) set_error(std::string(what) + ": refused: the channel count C (match: a multiple of 64 up to 960; merge / unmerge: a multiple of 8)");
    else if (rc == -3) set_error(std::string(what) + ": refused: a row stride below C or not a multiple of 8, a sample stride that is not a multiple of 8, or a base that is not 16-byte aligned");
    else if (rc == -4) set_error(std::string(what) + ": refused: more than 4096 dst tokens");
    else if (rc) set_error(std::string(what) + ": launch failed rc=" + std::to_string(rc));
    return rc;
}
long long ladi_op_tome_match_workspace_bytes(int n, int Ns, int Nd, int C) {
    if (n < 1 || Ns < 1 || Nd < 1 || C < 1) return -1;
    return (long long)n * ((long long)ladi_tome_pad_src(Ns) + ladi_tome_pad_dst(Nd)) * C * (long long)sizeof(h16);
}
long long ladi_op_tome_plan_ints(int Ns, int Nd, int r) { return ladi_tome_plan_ints(Ns, Nd, r); }
int ladi_op_tome_match(const void* x, int ld, long long sx, const int* src_pos, const int* dst_pos, int n, int T, int Ns, int Nd, int C,
                       void* workspace, float* score, int* node, void* stream) {
    if (!workspace || n < 1 || Ns < 1 || C < 1) return tome_op_rc("ladi_op_tome_match", -1);
    h16* A = reinterpret_cast<h16*>(workspace);
    h16* B = A + (size_t)n * ladi_tome_pad_src(Ns) * C;
    int rc = ladi_launch_tome_prep(reinterpret_cast<const h16*>(x), ld, sx, src_pos, dst_pos, n, T, Ns, Nd, C, A, B, S(stream));
    if (!rc) rc = score && node ? ladi_launch_tome_match(A, B, n, Ns, Nd, C, score, node, S(stream)) : -1;
    return tome_op_rc("ladi_op_tome_match", rc);
}
int ladi_op_tome_plan(const float* score, const int* node, const int* src_pos, const int* dst_pos, int n, int T, int Ns, int Nd, int r,
                      int* out_row, int* plan, void* stream) {
    return tome_op_rc("ladi_op_tome_plan", ladi_launch_tome_plan(score, node, src_pos, dst_pos, n, T, Ns, Nd, r, out_row, plan, S(stream)));
}
int ladi_op_tome_merge(const void* x, int ldx, long long sx, const int* dst_pos, const int* plan, int n, int T, int Ns, int Nd, int r, int C,
                       void* y, int ldy, long long sy, void* stream) {
    return tome_op_rc("ladi_op_tome_merge", ladi_launch_tome_merge(reinterpret_cast<const h16*>(x), ldx, sx, dst_pos, plan, n, T, Ns, Nd, r, C,
                                                                   reinterpret_cast<h16*>(y), ldy, sy, S(stream)));
}
int ladi_op_tome_unmerge_add(const void* y, int ldy, long long sy, const void* res, int ldr, long long sr, const int* out_row, int n, int T,
                             int Tm, int C, void* out, int ldo, long long so, void* stream) {
    return tome_op_rc("ladi_op_tome_unmerge_add", ladi_launch_tome_unmerge_add(reinterpret_cast<const h16*>(y), ldy, sy, reinterpret_cast<const h16*>(res),
                                                                               ldr, sr, out_row, n, T, Tm, C, reinterpret_cast<h16*>(out), ldo, so, S(stream)));
}

// ------------------------------------------------------------------------------------------------ LoRA (runtime_lora.cpp)
int ladi_unet_lora_load(ladi_unet* u, const char* name, const ladi_weights* ws) {
    return guarded("ladi_unet_lora_load", [&]() {
        if (!u || !name || !ws) throw std::runtime_error("null handle, name or weights");
        u->u.lora_load(name, ws->ws);
        return 0;
    });
}
int ladi_unet_set_adapters(ladi_unet* u, const char* const* names, const float* weights, int count, void* stream) {
    return guarded("ladi_unet_set_adapters", [&]() {
        if (!u) throw std::runtime_error("null handle");
        if (count < 0 || (count > 0 && (!names || !weights))) throw std::runtime_error("count < 0, or null names / weights with count > 0");
        std::vector<std::pair<std::string, float>> set;
        for (int i = 0; i < count; ++i) {
            if (!names[i]) throw std::runtime_error("null adapter name at index " + std::to_string(i));
            set.emplace_back(names[i], weights[i]);
        }
        u->u.lora_set(set, S(stream));
        return 0;
    });
}
int ladi_unet_lora_delete(ladi_unet* u, const char* name) {
    return guarded("ladi_unet_lora_delete", [&]() {
        if (!u || !name) throw std::runtime_error("null handle or name");
        u->u.lora_delete(name);
        return 0;
    });
}
int ladi_unet_lora_count(const ladi_unet* u) {
    if (!u) { set_error("ladi_unet_lora_count: null handle"); return -1; }
    return (int)u->u.lora_adapters.size();
}
const char* ladi_unet_lora_name(const ladi_unet* u, int i) {
    if (!u || i < 0 || i >= (int)u->u.lora_adapters.size()) { set_error("ladi_unet_lora_name: null handle or index out of range"); return nullptr; }
    return u->u.lora_adapters[i]->name.c_str();
}
int ladi_unet_lora_active(const ladi_unet* u, const char** names_out, float* weights_out, int cap) {
    if (!u || cap < 0 || (cap > 0 && (!names_out || !weights_out))) { set_error("ladi_unet_lora_active: null handle, cap < 0 or null outputs"); return -1; }
    const int n = (int)u->u.lora_active.size();
    for (int i = 0; i < n && i < cap; ++i) { names_out[i] = u->u.lora_active[i].first.c_str(); weights_out[i] = u->u.lora_active[i].second; }
    return n;
}
long long ladi_unet_export_weight(ladi_unet* u, const char* key, float* host_out, long long cap) {
    long long n = -1;
    const int rc = guarded("ladi_unet_export_weight", [&]() {
        if (!u || !key) throw std::runtime_error("null handle or key");
        if (host_out && cap < 0) throw std::runtime_error("cap < 0");
        n = u->u.export_weight(key, host_out, cap);
        return 0;
    });
    return rc ? -1 : n;
}
int ladi_op_lora_merge(const void* base, void* W, long long pitch, int cin, int cin_pad, int taps, int row0, int rows, int geglu_half,
                       int n_adapters, const float* const* up, const float* const* down, const int* rank, const float* scale,
                       unsigned* nonfinite, void* stream) {
    return guarded("ladi_op_lora_merge", [&]() {
        if (!base || !W || base == W) throw std::runtime_error("null base or W, or base == W");
        if (n_adapters < 0 || n_adapters > LORA_MAX_ADAPTERS) throw std::runtime_error("n_adapters " + std::to_string(n_adapters) + " outside [0, 8]");
        if (n_adapters > 0 && (!up || !down || !rank || !scale)) throw std::runtime_error("null up, down, rank or scale with n_adapters > 0");
        if (((uintptr_t)nonfinite & 3)) throw std::runtime_error("the non-finite counter is not 4-byte aligned");
        LoraMergeArgs a; std::memset(&a, 0, sizeof(a));
        a.base = reinterpret_cast<const h16*>(base); a.W = reinterpret_cast<h16*>(W); a.pitch = pitch;
        a.cin = cin; a.cin_pad = cin_pad; a.taps = taps; a.row0 = row0; a.rows = rows; a.geglu_half = geglu_half; a.n_adapters = n_adapters;
        for (int i = 0; i < n_adapters; ++i) {
            if (!std::isfinite(scale[i])) throw std::runtime_error("scale " + std::to_string(i) + " is not finite");
            a.up[i] = up[i]; a.down[i] = down[i]; a.rank[i] = rank[i]; a.scale[i] = scale[i];
        }
        a.nonfinite = nonfinite;
        const int rc = ladi_launch_lora_merge(a, S(stream));
        static const char* const why[] = {"", "null or identical base / W", "a size < 1, cin_pad < cin or cin_pad not a multiple of 64",
                                          "pitch below taps * cin_pad or not a multiple of 8, or base / W not 16-byte aligned",
                                          "GEGLU map: half not a multiple of 32, rows != 2 half or row0 not a multiple of 64", "more than 8 adapters",
                                          "a null or misaligned factor, or a rank outside [1, 256]", "grid too large"};
        if (rc) throw std::runtime_error(std::string("launch refused or failed (rc = ") + std::to_string(rc) + (rc <= -1 && rc >= -7 ? std::string("): ") + why[-rc] : ")"));
        return 0;
    });
}

// ------------------------------------------------------------------------------------------------ IP-Adapter (runtime_unet.cpp)
int ladi_unet_ip_adapter_load(ladi_unet* u, const ladi_weights* ws) {
    return guarded("ladi_unet_ip_adapter_load", [&]() {
        if (!u || !ws) throw std::runtime_error("null handle or weights");
        u->u.ip_load(ws->ws);
        return 0;
    });
}
int ladi_unet_ip_adapter_load_ex(ladi_unet* u, const ladi_weights* ws, int image_proj_dim_head) {
    return guarded("ladi_unet_ip_adapter_load_ex", [&]() {
        if (!u || !ws) throw std::runtime_error("null handle or weights");
        u->u.ip_load(ws->ws, image_proj_dim_head);
        return 0;
    });
}
int ladi_unet_ip_adapter_is_plus(const ladi_unet* u) {
    if (!u) { set_error("ladi_unet_ip_adapter_is_plus: null handle"); return -1; }
    return u->u.ip_resampler ? 1 : 0;
}
int ladi_unet_set_ip_context_seq(ladi_unet* u, const void* hidden, int n, int T, void* stream) {
    return guarded("ladi_unet_set_ip_context_seq", [&]() {
        if (!u) throw std::runtime_error("null handle");
        return u->u.set_ip_context_seq(reinterpret_cast<const h16*>(hidden), n, T, S(stream));
    });
}
int ladi_unet_ip_adapter_unload(ladi_unet* u) {
    return guarded("ladi_unet_ip_adapter_unload", [&]() {
        if (!u) throw std::runtime_error("null handle");
        HIP_OK(hipDeviceSynchronize());          // a forward still in flight may read the weights and the image K/V
        u->u.ip_unload();
        return 0;
    });
}
int ladi_unet_ip_adapter_info(const ladi_unet* u, int* tokens, int* embed_dim) {
    if (!u) { set_error("ladi_unet_ip_adapter_info: null handle"); return -1; }
    if (tokens) *tokens = u->u.ip_N;
    if (embed_dim) *embed_dim = u->u.ip_E;
    return u->u.ip_loaded ? 1 : 0;
}
int ladi_unet_set_ip_scale(ladi_unet* u, const float* scales, int count) {
    if (!u) { set_error("ladi_unet_set_ip_scale: null handle"); return -1; }
    try { u->u.ip_set_scale(scales, count); }
    catch (const std::exception& e) { set_error(std::string("ladi_unet_set_ip_scale: ") + e.what()); return -1; }
    return 0;
}
int ladi_unet_ip_scale(ladi_unet* u, float* scales_out, int cap) {
    if (!u || cap < 0 || (cap > 0 && !scales_out)) { set_error("ladi_unet_ip_scale: null handle, cap < 0 or null output"); return -1; }
    for (auto& b : u->u.xf) if (b.bit < cap) scales_out[b.bit] = b.ip_scale;
    return (int)u->u.xf.size();
}
int ladi_unet_set_ip_context(ladi_unet* u, const void* embeds, int n, void* stream) {
    return guarded("ladi_unet_set_ip_context", [&]() {
        if (!u) throw std::runtime_error("null handle");
        return u->u.set_ip_context(reinterpret_cast<const h16*>(embeds), n, S(stream));
    });
}
int ladi_unet_set_ip_tokens(ladi_unet* u, const void* tokens, int n, int N, void* stream) {
    return guarded("ladi_unet_set_ip_tokens", [&]() {
        if (!u) throw std::runtime_error("null handle");
        return u->u.set_ip_tokens(reinterpret_cast<const h16*>(tokens), n, N, S(stream));
    });
}
int ladi_unet_clear_ip_context(ladi_unet* u) {
    if (!u) { set_error("ladi_unet_clear_ip_context: null handle"); return -1; }
    u->u.clear_ip_context();
    return 0;
}
int ladi_unet_set_ip_route(ladi_unet* u, int route) {
    if (!u || route < 0 || route > 1) { set_error("ladi_unet_set_ip_route: null handle or a route other than 0 / 1"); return -1; }
    u->u.ip_route = route;
    return 0;
}
int ladi_op_ip_attn_add(const void* q, int ldq, long long sq, const void* k, int ldk, long long sk, const void* v, int ldv, long long sv, void* o,
                        int ldo, long long so, int n, int heads, int T, int N, float scale, void* stream) {
    const int rc = ladi_launch_ip_attn_add(reinterpret_cast<const h16*>(q), ldq, sq, reinterpret_cast<const h16*>(k), ldk, sk,
                                           reinterpret_cast<const h16*>(v), ldv, sv, reinterpret_cast<h16*>(o), ldo, so, n, heads, T, N, scale, S(stream));
    if (rc == -1)
        set_error("ladi_op_ip_attn_add: refused: a null pointer, n / heads / T < 1, N = " + std::to_string(N) + " outside [1, 64], a row stride that is "
                  "not a multiple of 8 or below heads * 64, a per-sample stride that is not a multiple of 8, or a base that is not 16-byte aligned");
    else if (rc) set_error("ladi_op_ip_attn_add: launch failed rc=" + std::to_string(rc));
    return rc;
}

int ladi_unet_forward_pag(ladi_unet* u, const void* sample, int dtype, int n, int h, int w, float timestep, void* out, int out_dtype,
                          int sample0, int pag_first, void* stream) {
    FwdOpt o; o.sample0 = sample0; o.pag_first = pag_first;
    return unet_forward_entry("ladi_unet_forward_pag", u, sample, dtype, n, h, w, timestep, out, out_dtype, o, stream, [&](UNet& U) {
        if (n < 1 || h < 1 || w < 1 || sample0 < 0 || sample0 + n > U.ctx_n)
            throw std::runtime_error("samples [" + std::to_string(sample0) + ", " + std::to_string(sample0 + n) + ") are not inside the context batch of " +
                                     std::to_string(U.ctx_n) + " (ladi_unet_set_context)");
        if (pag_first < 0) throw std::runtime_error("pag_first " + std::to_string(pag_first) + " is negative");
    }, [](UNet&) {});
}

int ladi_unet_forward(ladi_unet* u, const void* sample, int dtype, int n, int h, int w, float timestep, void* out, int out_dtype,
                      void* stream) {
    return unet_forward_entry("ladi_unet_forward", u, sample, dtype, n, h, w, timestep, out, out_dtype, FwdOpt(), stream, [&](UNet& U) {
        // the whole context batch: with an output view UNet::forward itself only asks for samples inside it
        if (n != U.ctx_n) throw std::runtime_error("UNet::forward: set_context batch mismatch");
    }, [](UNet&) {});
}

int ladi_unet_forward_cached_rows(ladi_unet* u, const void* sample, int dtype, int n, int h, int w, float timestep, void* out, int out_dtype,
                                  int mode, int branch, int sample0, void* stream) {
    FeatCache fc; fc.mode = mode; fc.branch = branch;
    FwdOpt o; o.sample0 = sample0; o.fc = mode ? &fc : nullptr;
    return unet_forward_entry("ladi_unet_forward_cached", u, sample, dtype, n, h, w, timestep, out, out_dtype, o, stream, [&](UNet& U) {
        if (mode < 0 || mode > 2) throw std::runtime_error("mode " + std::to_string(mode) + " unknown: 0 plain, 1 whole + capture, 2 shallow");
        if (mode && (branch < 0 || branch > U.cfg.layers_per_block))
            throw std::runtime_error("branch " + std::to_string(branch) + " out of range [0, " + std::to_string(U.cfg.layers_per_block) + "]");
        if (n < 1 || h < 1 || w < 1 || sample0 < 0 || sample0 + n > U.ctx_n)
            throw std::runtime_error("samples [" + std::to_string(sample0) + ", " + std::to_string(sample0 + n) + ") are not inside the context batch of " +
                                     std::to_string(U.ctx_n) + " (ladi_unet_set_context)");
        // every check of the cache comes before the first launch
        const bool same = U.fc_buf && U.fc_h == h && U.fc_w == w && U.fc_branch == branch;
        if (mode == FeatCache::SHALLOW) {
            bool ok = same && (int)U.fc_rows.size() >= sample0 + n;
            for (int i = 0; ok && i < n; ++i) ok = U.fc_rows[sample0 + i] != 0;
            if (!ok)
                throw std::runtime_error("shallow forward without a feature cache captured for samples [" + std::to_string(sample0) + ", " +
                                         std::to_string(sample0 + n) + ") at h = " + std::to_string(h) + ", w = " + std::to_string(w) + ", branch = " +
                                         std::to_string(branch) + " since the last ladi_unet_set_context (run mode 1 first)");
        }
        if (mode == FeatCache::CAPTURE) {
            const size_t need = (size_t)U.ctx_n * h * w * U.fc_channels(branch);
            if (!same) U.fc_rows.assign((size_t)U.ctx_n, 0);          // another geometry: what the cache held is gone
            if (need > U.fc_cap) {
                std::fill(U.fc_rows.begin(), U.fc_rows.end(), 0);
                if (U.fc_buf) HIP_OK(hipFree(U.fc_buf));
                U.fc_buf = nullptr; U.fc_cap = 0;
                HIP_OK(hipMalloc(reinterpret_cast<void**>(&U.fc_buf), need * sizeof(h16)));
                U.fc_cap = need;
            }
            U.fc_h = h; U.fc_w = w; U.fc_branch = branch;
        }
        fc.buf = U.fc_buf;
    }, [&](UNet& U) {
        if (mode == FeatCache::CAPTURE) for (int i = 0; i < n; ++i) U.fc_rows[sample0 + i] = 1;
    });
}

int ladi_unet_forward_cached(ladi_unet* u, const void* sample, int dtype, int n, int h, int w, float timestep, void* out, int out_dtype,
                             int mode, int branch, void* stream) {
    if (u && n != u->u.ctx_n) {
        set_error("ladi_unet_forward_cached: n = " + std::to_string(n) + " is not the context batch of " + std::to_string(u->u.ctx_n) +
                  " (ladi_unet_set_context); a cache captured at another n does not serve");
        return -2;
    }
    return ladi_unet_forward_cached_rows(u, sample, dtype, n, h, w, timestep, out, out_dtype, mode, branch, 0, stream);
}

// mode / branch: time the shallow forward (2) or the capturing one (1) against a scratch cache that holds zeros; 0: the plain forward
static int time_forward_any(const char* name, ladi_unet* u, int n, int h, int w, int iters, int mode, int branch, float* avg_ms, void* stream) {
    return guarded(name, [&]() {
        UNet& U = u->u;
        hipStream_t st = S(stream);
        if (mode < 0 || mode > 2 || (mode && (branch < 0 || branch > U.cfg.layers_per_block))) throw std::runtime_error("bad mode / branch");
        FeatCache fcs; fcs.mode = mode; fcs.branch = branch;
        struct Scratch { h16* p = nullptr; ~Scratch() { if (p) (void)hipFree(p); } } scratch;
        if (mode) {
            const size_t bytes = (size_t)n * h * w * U.fc_channels(branch) * sizeof(h16);
            HIP_OK(hipMalloc(reinterpret_cast<void**>(&scratch.p), bytes));
            HIP_OK(hipMemsetAsync(scratch.p, 0, bytes, st));
            fcs.buf = scratch.p;
        }
        FwdOpt fo; fo.fc = mode ? &fcs : nullptr;
        float t0 = 500.f;
        if (U.compute_temb(&t0, 1, st)) return -1;
        hipEvent_t e0, e1;
        HIP_OK(hipEventCreate(&e0)); HIP_OK(hipEventCreate(&e1));
        run_planned(U.arena, st, [&](Ctx& c) {
            Act x = c.new_act(n, h, w, 64);
            if (!c.dry()) HIP_OK(hipMemsetAsync(x.p, 0, x.pixels() * 64 * sizeof(h16), st));
            const size_t mk = c.ar->mark();
            // warm-up
            c.stats_off = 0; (void)U.forward(c, x, U.temb_table, nullptr, fo); c.ar->release(mk);
            if (!c.dry()) HIP_OK(hipEventRecord(e0, st));
            for (int i = 0; i < (c.dry() ? 1 : iters); ++i) {
                c.stats_off = 0;
                if (!c.dry() && c.stats_cap) HIP_OK(hipMemsetAsync(c.stats, 0, c.stats_cap * sizeof(float), st));
                (void)U.forward(c, x, U.temb_table, nullptr, fo);
                c.ar->release(mk);
            }
            if (!c.dry()) HIP_OK(hipEventRecord(e1, st));
        }, &U.stats, &U.stats_cap);
        HIP_OK(hipEventSynchronize(e1));
        float ms = 0.f;
        HIP_OK(hipEventElapsedTime(&ms, e0, e1));
        *avg_ms = ms / (float)iters;
        (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
        return 0;
    });
}
int ladi_unet_time_forward(ladi_unet* u, int n, int h, int w, int iters, float* avg_ms, void* stream) {
    return time_forward_any("ladi_unet_time_forward", u, n, h, w, iters, 0, 0, avg_ms, stream);
}
int ladi_unet_time_forward_cached(ladi_unet* u, int n, int h, int w, int iters, int mode, int branch, float* avg_ms, void* stream) {
    return time_forward_any("ladi_unet_time_forward_cached", u, n, h, w, iters, mode, branch, avg_ms, stream);
}

int ladi_unet_time_forward_lanes(ladi_unet* u, int n, int h, int w, int iters, int lanes, int use_graph, float* avg_ms, void* stream) {
    return guarded("ladi_unet_time_forward_lanes", [&]() {
        UNet& U = u->u;
        UNetLanes& LN = u->lanes;
        if (iters < 1 || n < 1) throw std::runtime_error("bad arguments");
        hipStream_t user = S(stream), st = nullptr;
        HIP_OK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));      // the NULL stream cannot be captured
        hipEvent_t e0 = nullptr, e1 = nullptr, ein = nullptr;
        GraphTable graphs;      // slot 0: the one forward
        auto cleanup = [&]() {
            graphs.clear();
            if (e0) (void)hipEventDestroy(e0);
            if (e1) (void)hipEventDestroy(e1);
            if (ein) (void)hipEventDestroy(ein);
            (void)hipStreamSynchronize(st); (void)hipStreamDestroy(st);
        };
        try {
            HIP_OK(hipEventCreate(&e0)); HIP_OK(hipEventCreate(&e1)); HIP_OK(hipEventCreateWithFlags(&ein, hipEventDisableTiming));
            HIP_OK(hipEventRecord(ein, user)); HIP_OK(hipStreamWaitEvent(st, ein, 0));
            float t0 = 500.f;
            if (U.compute_temb(&t0, 1, st)) throw std::runtime_error("time embedding failed");   // (a throw, so that cleanup() runs: ADVICE r04)
            LN.configure(n, lanes > 0 ? lanes : 0);
            const int eps_ld = (U.cfg.out_channels + 3) / 4 * 4;
            Arena& io = u->io;
            Act x, eps;
            run_planned(io, st, [&](Ctx& c) {
                x = c.new_act(n, h, w, 64);
                eps = c.new_act(n, h, w, U.cfg.out_channels, eps_ld);
                if (c.dry()) { LN.forward(U, st, true, false, x, eps, U.temb_table, nullptr); LN.commit_plan(); }
            });
            HIP_OK(hipMemsetAsync(x.p, 0, x.pixels() * 64 * sizeof(h16), st));
            LN.forward(U, st, false, false, x, eps, U.temb_table, nullptr);      // warm-up, lanes in sequence (tile measurement)
            if (use_graph) {
                graphs.capture(0, st, [&]() { LN.forward(U, st, false, true, x, eps, U.temb_table, nullptr); });
                HIP_OK(hipGraphLaunch(graphs.e[0], st));                        // one untimed replay
            } else LN.forward(U, st, false, true, x, eps, U.temb_table, nullptr);
            HIP_OK(hipEventRecord(e0, st));
            for (int i = 0; i < iters; ++i) {
                if (use_graph) HIP_OK(hipGraphLaunch(graphs.e[0], st));
                else LN.forward(U, st, false, true, x, eps, U.temb_table, nullptr);
            }
            HIP_OK(hipEventRecord(e1, st));
            HIP_OK(hipEventSynchronize(e1));
            float ms = 0.f;
            HIP_OK(hipEventElapsedTime(&ms, e0, e1));
            *avg_ms = ms / (float)iters;
        } catch (...) { cleanup(); throw; }
        cleanup();
        return 0;
    });
}

// ------------------------------------------------------------------------------------------------ VAE
ladi_vae* ladi_vae_create(const ladi_vae_config* cfg, const ladi_weights* ws) {
    ladi_vae* h = nullptr;
    int rc = guarded("ladi_vae_create", [&]() {
        if (!cfg || !ws) throw std::runtime_error("null argument");
        require_gpu();
        VAECfg c;
        c.in_channels = cfg->in_channels; c.out_channels = cfg->out_channels; c.latent_channels = cfg->latent_channels;
        for (int i = 0; i < 4; ++i) c.boc[i] = cfg->block_out_channels[i];
        c.layers_per_block = cfg->layers_per_block; c.groups = cfg->norm_num_groups; c.scaling_factor = cfg->scaling_factor;
        if (c.latent_channels != 4 || c.in_channels != 3 || c.out_channels != 3) throw std::runtime_error("VAE: only 3->4->3 channels supported");
        h = new ladi_vae();
        h->v.load(c, ws->ws);
        return 0;
    });
    if (rc) { delete h; return nullptr; }
    return h;
}
void ladi_vae_destroy(ladi_vae* v) { if (v) set_module_probe(v->v.probe, nullptr); delete v; }

int ladi_vae_encode(ladi_vae* v, const void* x, int dtype, int B, int H, int W, float* moments, void* const* feats_out, void* stream) {
    return guarded("ladi_vae_encode", [&]() {
        VAE& V = v->v;
        hipStream_t st = S(stream);
        if (H % 8 || W % 8) throw std::runtime_error("H and W must be divisible by 8");
        run_planned(V.arena, st, [&](Ctx& c) {
            Act xi = c.new_act(B, H, W, 64);
            if (!c.dry()) c.check(ladi_launch_nchw_to_nhwc(x, dtype == LADI_F32, B, 3, H, W, xi.p, 64, st), "nchw_to_nhwc");
            Act feats[5];
            c.bad = V.d_bad;
            Act mom = V.encode(c, xi, feats);
            c.bad = nullptr;
            if (c.dry()) return;
            c.check(ladi_launch_nhwc_to_nchw(mom.p, mom.ld, B, 8, H / 8, W / 8, moments, 1, st), "moments");
            if (feats_out)
                for (int i = 0; i < 5; ++i)
                    if (feats_out[i]) HIP_OK(hipMemcpyAsync(feats_out[i], feats[i].p, feats[i].pixels() * feats[i].c * sizeof(h16), hipMemcpyDeviceToDevice, st));
        }, &V.stats, &V.stats_cap);
        // the encoder's intermediate features feed EMASC at their true scale, so there is no scaled form to fall back to: report instead
        if (V.overflowed(st)) throw std::runtime_error("VAE encode: activations exceed the fp16 range (non-finite GroupNorm statistics)");
        return 0;
    });
}

int ladi_vae_decode(ladi_vae* v, const float* z, int B, int h, int w, const void* const* skips_dev, void* sample, int out_dtype,
                    void* stream) {
    return guarded("ladi_vae_decode", [&]() {
        VAE& V = v->v;
        hipStream_t st = S(stream);
        (void)V.decode_guarded(st, [&](int shift) {
        run_planned(V.arena, st, [&](Ctx& c) {
            float* zp = c.alloc_f32((size_t)B * h * w * 4);
            Act zi = c.new_act(B, h, w, 64);
            Act skips[5];
            if (skips_dev) {
                const int H = 8 * h, W = 8 * w;
                const int sh[5] = {H, H, H / 2, H / 4, H / 8}, sw[5] = {W, W, W / 2, W / 4, W / 8};
                const int sc[5] = {V.cfg.boc[0], V.cfg.boc[1], V.cfg.boc[2], V.cfg.boc[3], V.cfg.boc[3]};
                for (int i = 0; i < 5; ++i) {
                    if (!skips_dev[i]) continue;                      // slot omitted by the int_layers selection
                    skips[i].p = reinterpret_cast<h16*>(const_cast<void*>(skips_dev[i]));
                    skips[i].n = B; skips[i].h = sh[i]; skips[i].w = sw[i]; skips[i].c = sc[i]; skips[i].ld = sc[i];
                }
            }
            if (!c.dry()) {
                c.check(ladi_launch_lat_nchw_to_pix(z, B, h * w, 1.0f, zp, st), "z");
                c.check(ladi_launch_post_quant(zp, V.d_pq, 1.0f, B * h * w, zi.p, 64, st), "post_quant");
            }
            Act img = V.decode(c, zi, skips_dev ? skips : nullptr, shift);
            if (!c.dry()) c.check(ladi_launch_nhwc_to_nchw(img.p, img.ld, B, 3, 8 * h, 8 * w, sample, out_dtype == LADI_F32, st), "sample");
        }, &V.stats, &V.stats_cap);
        });
        return 0;
    });
}

int ladi_vae_set_range_shift(ladi_vae* v, int shift) {
    if (!v || shift > 12) { set_error("ladi_vae_set_range_shift: shift must be -1 (automatic) or 0..12"); return -1; }
    v->v.range_shift = shift < 0 ? -1 : shift;
    return 0;
}
int ladi_vae_last_range_shift(const ladi_vae* v) { return v ? v->v.last_shift : -1; }

// ------------------------------------------------------------------------------------------------ EMASC
ladi_emasc* ladi_emasc_create(const ladi_emasc_config* cfg, const ladi_weights* ws) {
    ladi_emasc* h = nullptr;
    int rc = guarded("ladi_emasc_create", [&]() {
        if (!cfg || !ws) throw std::runtime_error("null argument");
        require_gpu();
        if (cfg->n < 1 || cfg->n > 8) throw std::runtime_error("EMASC: n out of range");
        EMASCCfg c; c.n = cfg->n;
        for (int i = 0; i < cfg->n; ++i) { c.in_ch[i] = cfg->in_channels[i]; c.out_ch[i] = cfg->out_channels[i]; }
        h = new ladi_emasc();
        h->e.load(c, ws->ws);
        return 0;
    });
    if (rc) { delete h; return nullptr; }
    return h;
}
void ladi_emasc_destroy(ladi_emasc* e) { if (e) set_module_probe(e->e.probe, nullptr); delete e; }

int ladi_emasc_forward(ladi_emasc* e, const void* const* feats_dev, const int* hs, const int* wss, int B, const void* mask_dev, int Hm,
                       int Wm, void* const* outs_dev, void* stream) {
    return guarded("ladi_emasc_forward", [&]() {
        EMASC& E = e->e;
        hipStream_t st = S(stream);
        run_planned(E.arena, st, [&](Ctx& c) {
            Act feats[8], outs[8];
            const h16* masks[8];
            for (int i = 0; i < E.cfg.n; ++i) {
                feats[i].p = reinterpret_cast<h16*>(const_cast<void*>(feats_dev[i]));
                feats[i].n = B; feats[i].h = hs[i]; feats[i].w = wss[i]; feats[i].c = E.cfg.in_ch[i]; feats[i].ld = E.cfg.in_ch[i];
                outs[i] = feats[i]; outs[i].p = reinterpret_cast<h16*>(outs_dev[i]); outs[i].c = E.cfg.out_ch[i]; outs[i].ld = E.cfg.out_ch[i];
                masks[i] = nullptr;
                if (mask_dev) {
                    const int s = Hm / hs[i];
                    if (s * hs[i] != Hm || s * wss[i] != Wm) throw std::runtime_error("EMASC: mask size must be an integer multiple of each feature size");
                    if (s == 1) masks[i] = reinterpret_cast<const h16*>(mask_dev);
                    else {
                        h16* m = c.alloc_h16((size_t)B * hs[i] * wss[i]);
                        if (!c.dry()) c.check(ladi_launch_mask_down(reinterpret_cast<const h16*>(mask_dev), B, Hm, Wm, s, m, st), "mask_down");
                        masks[i] = m;
                    }
                }
            }
            E.forward(c, feats, mask_dev ? masks : nullptr, outs, true);
        });
        return 0;
    });
}

int ladi_mask_features(void* feat, int B, int h, int w, int C, const void* mask, int Hm, int Wm, void* stream) {
    return guarded("ladi_mask_features", [&]() {
        hipStream_t st = S(stream);
        const int s = Hm / h;
        if (s * h != Hm || s * w != Wm) throw std::runtime_error("mask size must be an integer multiple of the feature size");
        const h16* m = reinterpret_cast<const h16*>(mask);
        h16* tmp = nullptr;
        if (s != 1) {
            HIP_OK(hipMallocAsync(reinterpret_cast<void**>(&tmp), (size_t)B * h * w * sizeof(h16), st));
            int rc = ladi_launch_mask_down(m, B, Hm, Wm, s, tmp, st);
            if (rc) return rc;
            m = tmp;
        }
        int rc = ladi_launch_mask_mul(reinterpret_cast<h16*>(feat), C, B * h * w, m, st);
        if (tmp) HIP_OK(hipFreeAsync(tmp, st));
        return rc;
    });
}

// ------------------------------------------------------------------------------------------------ adapter
ladi_adapter* ladi_adapter_create(const ladi_adapter_config* cfg, const ladi_weights* ws) {
    ladi_adapter* h = nullptr;
    int rc = guarded("ladi_adapter_create", [&]() {
        if (!cfg || !ws) throw std::runtime_error("null argument");
        require_gpu();
        AdapterCfg c; c.hidden = cfg->hidden; c.heads = cfg->heads; c.mlp = cfg->mlp_dim; c.head_hidden = cfg->head_hidden; c.out_dim = cfg->out_dim;
        c.ln_eps = cfg->layer_norm_eps;
        if (c.hidden % 64 || c.hidden / c.heads > 128) throw std::runtime_error("adapter: hidden must be a multiple of 64 and head dim <= 128");
        h = new ladi_adapter();
        h->a.load(c, ws->ws);
        return 0;
    });
    if (rc) { delete h; return nullptr; }
    return h;
}
void ladi_adapter_destroy(ladi_adapter* a) { delete a; }
int ladi_adapter_forward(ladi_adapter* a, const void* x, int B, int T, void* out, void* stream) {
    return guarded("ladi_adapter_forward", [&]() { return a->a.forward(reinterpret_cast<const h16*>(x), B, T, reinterpret_cast<h16*>(out), S(stream)); });
}

// ------------------------------------------------------------------------------------------------ text encoder
ladi_text_encoder* ladi_text_encoder_create(const ladi_text_config* cfg, const ladi_weights* ws) {
    ladi_text_encoder* h = nullptr;
    int rc = guarded("ladi_text_encoder_create", [&]() {
        if (!cfg || !ws) throw std::runtime_error("null argument");
        require_gpu();
        TextCfg c; c.vocab = cfg->vocab_size; c.hidden = cfg->hidden; c.heads = cfg->heads; c.mlp = cfg->mlp_dim; c.layers = cfg->layers;
        c.max_pos = cfg->max_positions; c.vstar_id = cfg->vstar_token_id; c.ln_eps = cfg->layer_norm_eps;
        if (c.layers <= 0 || c.heads <= 0 || c.hidden % 64 || c.mlp % 64) throw std::runtime_error("text encoder: bad config");
        h = new ladi_text_encoder();
        h->t.load(c, ws->ws);
        return 0;
    });
    if (rc) { delete h; return nullptr; }
    return h;
}
void ladi_text_encoder_destroy(ladi_text_encoder* t) { delete t; }
int ladi_text_encoder_forward(ladi_text_encoder* t, const int* ids, int B, int T, const void* wemb, int nv, void* out_hidden, void* out_pooled,
                              void* stream) {
    return guarded("ladi_text_encoder_forward", [&]() {
        if (!t || !ids || !out_hidden) throw std::runtime_error("null argument");
        if (wemb && nv <= 0) throw std::runtime_error("num_vstar must be positive when word embeddings are given");
        return t->t.forward(ids, 0, B, T, reinterpret_cast<const h16*>(wemb), nv, reinterpret_cast<h16*>(out_hidden), reinterpret_cast<h16*>(out_pooled), S(stream));
    });
}
int ladi_text_encoder_forward_dev(ladi_text_encoder* t, const int* ids_dev, int B, int T, const void* wemb, int nv, void* out_hidden, void* out_pooled,
                                  void* stream) {
    return guarded("ladi_text_encoder_forward_dev", [&]() {
        if (!t || !ids_dev || !out_hidden) throw std::runtime_error("null argument");
        if (wemb && nv <= 0) throw std::runtime_error("num_vstar must be positive when word embeddings are given");
        return t->t.forward(ids_dev, 1, B, T, reinterpret_cast<const h16*>(wemb), nv, reinterpret_cast<h16*>(out_hidden), reinterpret_cast<h16*>(out_pooled), S(stream));
    });
}

// ------------------------------------------------------------------------------------------------ vision encoder
ladi_vision_encoder* ladi_vision_encoder_create(const ladi_vision_config* cfg, const ladi_weights* ws) {
    ladi_vision_encoder* h = nullptr;
    int rc = guarded("ladi_vision_encoder_create", [&]() {
        if (!cfg || !ws) throw std::runtime_error("null argument");
        require_gpu();
        VisionCfg c; c.hidden = cfg->hidden; c.heads = cfg->heads; c.mlp = cfg->mlp_dim; c.layers = cfg->layers; c.image = cfg->image_size;
        c.patch = cfg->patch_size; c.ln_eps = cfg->layer_norm_eps;
        if (c.layers <= 0 || c.heads <= 0 || c.patch <= 0 || c.hidden % 32 || c.mlp % 32) throw std::runtime_error("vision encoder: bad config");
        h = new ladi_vision_encoder();
        h->v.load(c, ws->ws);
        return 0;
    });
    if (rc) { delete h; return nullptr; }
    return h;
}
void ladi_vision_encoder_destroy(ladi_vision_encoder* v) { delete v; }
int ladi_vision_encoder_forward(ladi_vision_encoder* v, const void* px, int dtype, int B, void* out_hidden, void* out_pooled, void* stream) {
    return guarded("ladi_vision_encoder_forward", [&]() {
        if (!v || !px || !out_hidden) throw std::runtime_error("null argument");
        if (dtype != 0 && dtype != 1) throw std::runtime_error("pixel_values dtype must be fp32 (0) or fp16 (1)");
        return v->v.forward(px, dtype == 0, B, reinterpret_cast<h16*>(out_hidden), reinterpret_cast<h16*>(out_pooled), S(stream));
    });
}

int ladi_vision_encoder_projection_dim(const ladi_vision_encoder* v) {
    if (!v) { set_error("ladi_vision_encoder_projection_dim: null handle"); return -1; }
    return v->v.proj_dim;
}
int ladi_vision_encoder_forward_ex(ladi_vision_encoder* v, const void* px, int dtype, int B, void* out_hidden, void* out_pooled,
                                   void* out_penultimate, void* out_image_embeds, void* stream) {
    return guarded("ladi_vision_encoder_forward_ex", [&]() {
        if (!v || !px) throw std::runtime_error("null argument");
        if (dtype != 0 && dtype != 1) throw std::runtime_error("pixel_values dtype must be fp32 (0) or fp16 (1)");
        return v->v.forward_ex(px, dtype == 0, B, reinterpret_cast<h16*>(out_hidden), reinterpret_cast<h16*>(out_pooled),
                               reinterpret_cast<h16*>(out_penultimate), reinterpret_cast<h16*>(out_image_embeds), S(stream));
    });
}

// ------------------------------------------------------------------------------------------------ Resampler (IP-Adapter Plus image projection)
ladi_resampler* ladi_resampler_create(const ladi_weights* ws, int dim_head) {
    ladi_resampler* h = nullptr;
    int rc = guarded("ladi_resampler_create", [&]() {
        if (!ws) throw std::runtime_error("null weights");
        // the geometry and every limit are checked on the host first (Resampler::load), so a refusal needs no device
        std::unique_ptr<ladi_resampler> r(new ladi_resampler());
        r->r.check(ws->ws, "", dim_head);
        require_gpu();
        r->r.upload(ws->ws, "");
        h = r.release();
        return 0;
    });
    if (rc) return nullptr;
    return h;
}
void ladi_resampler_destroy(ladi_resampler* r) { delete r; }
int ladi_resampler_info(const ladi_resampler* r, int* N, int* E, int* dim, int* depth, int* heads, int* out_dim) {
    if (!r) { set_error("ladi_resampler_info: null handle"); return -1; }
    if (N) *N = r->r.N;
    if (E) *E = r->r.E;
    if (dim) *dim = r->r.dim;
    if (depth) *depth = r->r.depth;
    if (heads) *heads = r->r.heads;
    if (out_dim) *out_dim = r->r.out_dim;
    return 0;
}
int ladi_resampler_forward(ladi_resampler* r, const void* x, int n, int T, void* tokens_out, void* stream) {
    return guarded("ladi_resampler_forward", [&]() {
        if (!r) throw std::runtime_error("null handle");
        r->r.forward(reinterpret_cast<const h16*>(x), n, T, reinterpret_cast<h16*>(tokens_out), S(stream));
        return 0;
    });
}

// ------------------------------------------------------------------------------------------------ refinement UNet
ladi_refine* ladi_refine_create(const ladi_refine_config* cfg, const ladi_weights* ws) {
    ladi_refine* h = nullptr;
    int rc = guarded("ladi_refine_create", [&]() {
        if (!cfg || !ws) throw std::runtime_error("null argument");
        require_gpu();
        RefineCfg c; c.in_ch = cfg->in_channels; c.out_ch = cfg->out_channels; c.base = cfg->base_channels; c.bn_eps = cfg->bn_eps;
        h = new ladi_refine();
        h->r.load(c, ws->ws);
        return 0;
    });
    if (rc) { delete h; return nullptr; }
    return h;
}
void ladi_refine_destroy(ladi_refine* r) { delete r; }
int ladi_refine_forward(ladi_refine* r, const void* x, int dtype, int B, int H, int W, void* out, int out_dtype, void* stream) {
    return guarded("ladi_refine_forward", [&]() {
        if (!r || !x || !out) throw std::runtime_error("null argument");
        if ((dtype != 0 && dtype != 1) || (out_dtype != 0 && out_dtype != 1)) throw std::runtime_error("dtype must be fp32 (0) or fp16 (1)");
        return r->r.forward(x, dtype == 0, B, H, W, out, out_dtype == 0, S(stream));
    });
}

// ------------------------------------------------------------------------------------------------ TPS matching network
ladi_tps* ladi_tps_create(const ladi_tps_config* cfg, const ladi_weights* ws) {
    ladi_tps* h = nullptr;
    int rc = guarded("ladi_tps_create", [&]() {
        if (!cfg || !ws) throw std::runtime_error("null argument");
        require_gpu();
        TpsCfg c; c.height = cfg->height; c.width = cfg->width; c.input_nc = cfg->input_nc; c.n_layers = cfg->n_layers; c.grid = cfg->grid_size;
        c.ngf = cfg->ngf; c.bn_eps = cfg->bn_eps;
        if (c.n_layers != 3 || c.ngf != 64) throw std::runtime_error("TPS: only the released topology (n_layer = 3, ngf = 64) is supported");
        h = new ladi_tps();
        h->t.load(c, ws->ws);
        return 0;
    });
    if (rc) { delete h; return nullptr; }
    return h;
}
void ladi_tps_destroy(ladi_tps* t) { delete t; }
int ladi_tps_forward(ladi_tps* t, const void* a, const void* b, int dtype, int B, float* grid, float* coor, void* stream) {
    return guarded("ladi_tps_forward", [&]() {
        if (!t || !a || !b || !grid) throw std::runtime_error("null argument");
        if (dtype != 0 && dtype != 1) throw std::runtime_error("dtype must be fp32 (0) or fp16 (1)");
        return t->t.forward(a, b, dtype == 0, B, grid, coor, S(stream));
    });
}

// ------------------------------------------------------------------------------------------------ scheduler helpers
int ladi_sched_timesteps(int kind, int steps, int* out, int cap) {
    return guarded("ladi_sched_timesteps", [&]() {
        std::vector<float> ac; default_alphas_cumprod(ac);
        const SchedCode sc = decode_sched_code(kind);
        const int k = sc.kind;
        // (the step-count range is the table builder's: it depends on the code; trailing Euler timesteps are integers)
        if (!sc.trailing && (k == SCHED_LMS || k == SCHED_EULER || k == SCHED_EULER_A))
            throw std::runtime_error("LMSDiscrete / EulerDiscrete / EulerAncestralDiscrete timesteps are fractional: use ladi_sched_lms");
        std::vector<double> ts; std::vector<StepTable> tb;
        build_step_table(kind, steps, ac.data(), 1 << 30, ts, tb);
        if ((int)ts.size() > cap) throw std::runtime_error("timesteps buffer too small");
        for (size_t i = 0; i < ts.size(); ++i) out[i] = (int)ts[i];
        return (int)ts.size();
    });
}
int ladi_sched_lms(int steps, const float* ac_host, double* timesteps_out, float* sigmas_out, float* coeffs_out) {
    return guarded("ladi_sched_lms", [&]() {
        if (steps < 2 || steps > 1000) throw std::runtime_error("num_inference_steps out of range");
        std::vector<float> ac;
        if (ac_host) ac.assign(ac_host, ac_host + 1000); else default_alphas_cumprod(ac);
        std::vector<double> ts; std::vector<StepTable> tb; SchedInfo info;
        build_step_table(2, steps, ac.data(), 1 << 30, ts, tb, &info);
        if (timesteps_out) std::memcpy(timesteps_out, ts.data(), ts.size() * sizeof(double));
        if (sigmas_out) std::memcpy(sigmas_out, info.sigmas.data(), info.sigmas.size() * sizeof(float));
        if (coeffs_out) std::memcpy(coeffs_out, info.lms_coeffs.data(), info.lms_coeffs.size() * sizeof(float));
        return steps;
    });
}
static int sched_table_any(const char* name, int code, int steps, const float* ac_host, double* timesteps_out, float* rows_out, int cap,
                           float eta, int first_step = 0, float* start_out = nullptr) {
    return guarded(name, [&]() {
        std::vector<float> ac;
        if (ac_host) ac.assign(ac_host, ac_host + 1000); else default_alphas_cumprod(ac);
        std::vector<double> ts; std::vector<StepTable> tb; SchedInfo info;
        build_step_table(code, steps, ac.data(), 1 << 30, ts, tb, &info, eta, first_step);
        if ((int)tb.size() > cap) throw std::runtime_error("table buffer too small");
        if (start_out) { start_out[0] = info.start_kx; start_out[1] = info.start_kn; start_out[2] = info.in_scale0; }
        for (size_t i = 0; i < tb.size(); ++i) {
            const StepTable& e = tb[i];
            const float row[10] = {e.c_x, e.c_e, e.w[0], e.w[1], e.w[2], e.w[3], e.p_x, e.p_e, e.c_n, e.in_scale_next};
            if (rows_out) std::memcpy(rows_out + 10 * i, row, sizeof(row));
            if (timesteps_out) timesteps_out[i] = ts[i];
        }
        return (int)tb.size();
    });
}
int ladi_sched_table(int code, int steps, const float* ac_host, double* timesteps_out, float* rows_out, int cap) {
    return sched_table_any("ladi_sched_table", code, steps, ac_host, timesteps_out, rows_out, cap, 0.f);
}
int ladi_sched_table_eta(int code, int steps, const float* ac_host, float eta, double* timesteps_out, float* rows_out, int cap) {
    return sched_table_any("ladi_sched_table_eta", code, steps, ac_host, timesteps_out, rows_out, cap, eta);
}
int ladi_sched_table_from(int code, int steps, const float* ac_host, float eta, int first_step, double* timesteps_out, float* rows_out, int cap,
                          float* start_out) {
    return sched_table_any("ladi_sched_table_from", code, steps, ac_host, timesteps_out, rows_out, cap, eta, first_step, start_out);
}
int ladi_sched_keep_coeffs(int code, int steps, const float* ac_host, int first_step, float* out, int cap) {
    return guarded("ladi_sched_keep_coeffs", [&]() {
        if (!out) throw std::runtime_error("null out");
        std::vector<float> ac;
        if (ac_host) ac.assign(ac_host, ac_host + 1000); else default_alphas_cumprod(ac);
        std::vector<float> kt;
        build_keep_coeffs(code, steps, ac.data(), first_step, kt);
        const int evals = (int)(kt.size() / 2);
        if (evals > cap) throw std::runtime_error("coefficient buffer too small");
        std::memcpy(out, kt.data(), kt.size() * sizeof(float));
        return evals;
    });
}
int ladi_sched_alphas_cumprod(float* out) {
    std::vector<float> ac; default_alphas_cumprod(ac);
    std::memcpy(out, ac.data(), 1000 * sizeof(float));
    return 0;
}

// ------------------------------------------------------------------------------------------------ try-on
ladi_tryon* ladi_tryon_create(ladi_unet* unet, ladi_vae* vae, ladi_emasc* emasc) {
    if (!unet || !vae) { set_error("ladi_tryon_create: unet and vae required"); return nullptr; }
    ladi_tryon* t = new (std::nothrow) ladi_tryon();
    if (!t) return nullptr;
    t->t.unet = &unet->u; t->t.vae = &vae->v; t->t.emasc = emasc ? &emasc->e : nullptr;
    return t;
}
void ladi_tryon_destroy(ladi_tryon* t) { delete t; }
static int tryon_run_any(ladi_tryon* t, const ladi_tryon_inputs* in, void* images, int images_u8, float* latents, void* stream) {
    return guarded(images_u8 ? "ladi_tryon_run_u8" : "ladi_tryon_run", [&]() {
        if (!t || !in || !images) throw std::runtime_error("null argument");
        TryOnInputs ti;
        ti.batch = in->batch; ti.height = in->height; ti.width = in->width; ti.in_f32 = in->in_dtype == LADI_F32;
        ti.image = in->image_dev; ti.mask_image = in->mask_image_dev; ti.pose_map = in->pose_map_dev; ti.warped_cloth = in->warped_cloth_dev;
        ti.pose_channels = in->pose_channels;
        ti.prompt_embeds = reinterpret_cast<const h16*>(in->prompt_embeds_dev);
        ti.negative_prompt_embeds = reinterpret_cast<const h16*>(in->negative_prompt_embeds_dev);
        ti.L = in->L;
        ti.noise_cloth = in->noise_cloth_dev; ti.noise_latents = in->noise_latents_dev; ti.noise_masked = in->noise_masked_dev;
        ti.steps = in->num_inference_steps; ti.guidance = in->guidance_scale; ti.scheduler = in->scheduler;
        ti.cloth_zero_from = in->cloth_zero_from_eval; ti.no_pose = in->no_pose; ti.use_graph = in->use_graph;
        ti.alphas_cumprod = in->alphas_cumprod_host;
        // (the lower bound per scheduler code, 2 or 1, is the step-table builder's)
        if (ti.steps < 1 || ti.steps > 1000) throw std::runtime_error("num_inference_steps out of range");
        if (!ti.image || !ti.mask_image || !ti.pose_map || !ti.prompt_embeds || !ti.noise_latents || !ti.noise_masked) throw std::runtime_error("missing input");
        if (ti.warped_cloth && !ti.noise_cloth) throw std::runtime_error("noise_cloth required with warped_cloth");
        return t->t.run(ti, images, images_u8, latents, S(stream));
    });
}
int ladi_tryon_run(ladi_tryon* t, const ladi_tryon_inputs* in, float* images, float* latents, void* stream) {
    return tryon_run_any(t, in, images, 0, latents, stream);
}
int ladi_tryon_run_u8(ladi_tryon* t, const ladi_tryon_inputs* in, unsigned char* images, float* latents, void* stream) {
    return tryon_run_any(t, in, images, 1, latents, stream);
}
int ladi_tryon_stage_ms(ladi_tryon* t, float* out3) { return t ? t->t.stage_ms(out3) : -1; }
int ladi_tryon_poll_overflow(ladi_tryon* t) {
    if (!t || !t->t.vae) { set_error("ladi_tryon_poll_overflow: null handle"); return -1; }
    return guarded("ladi_tryon_poll_overflow", [&]() { return t->t.vae->poll_overflow(); });
}
int ladi_tryon_set_lanes(ladi_tryon* t, int lanes) {
    if (!t || lanes < 0 || lanes > UNetLanes::MAXG) { set_error("ladi_tryon_set_lanes: lanes must be in [0, 8]"); return -1; }
    t->t.lanes_override = lanes;
    return 0;
}
int ladi_tryon_lanes(ladi_tryon* t) { return t ? t->t.lanes.G : -1; }
int ladi_tryon_set_step_noise(ladi_tryon* t, const float* noise_dev, int steps) {
    if (!t || steps < 0) { set_error("ladi_tryon_set_step_noise: null handle or negative steps"); return -1; }
    t->t.step_noise_src = noise_dev; t->t.step_noise_steps = noise_dev ? steps : 0;
    return 0;
}
int ladi_tryon_set_init(ladi_tryon* t, const float* init_latents_dev, int hs, int ws, int first_step, int noisy) {
    if (!t) { set_error("ladi_tryon_set_init: null handle"); return -1; }
    if (first_step < 0) { set_error("ladi_tryon_set_init: first_step " + std::to_string(first_step) + " is negative"); return -1; }
    if (!init_latents_dev || first_step == 0) {
        t->t.init_src = nullptr; t->t.init_hs = t->t.init_ws = t->t.init_first = t->t.init_noisy = 0;
        return 0;
    }
    if (hs < 1 || ws < 1 || hs > 8192 || ws > 8192) {
        set_error("ladi_tryon_set_init: init latents of size " + std::to_string(hs) + " x " + std::to_string(ws) + " (each side has to be in [1, 8192])");
        return -1;
    }
    t->t.init_src = init_latents_dev; t->t.init_hs = hs; t->t.init_ws = ws; t->t.init_first = first_step; t->t.init_noisy = noisy ? 1 : 0;
    return 0;
}
int ladi_tryon_set_eta(ladi_tryon* t, float eta) {
    if (!t || !(eta >= 0.f) || !std::isfinite(eta)) { set_error("ladi_tryon_set_eta: null handle, or eta not finite and >= 0"); return -1; }
    t->t.eta = eta;
    return 0;
}
int ladi_tryon_set_guidance_schedule(ladi_tryon* t, const float* scales_host, int count) {
    if (!t || count < 0) { set_error("ladi_tryon_set_guidance_schedule: null handle or negative count"); return -1; }
    if (!scales_host || count == 0) { t->t.g_sched.clear(); return 0; }
    for (int i = 0; i < count; ++i)
        if (!std::isfinite(scales_host[i]) || scales_host[i] < 0.f) {
            set_error("ladi_tryon_set_guidance_schedule: entry " + std::to_string(i) + " is negative or not finite");
            return -1;
        }
    return guarded("ladi_tryon_set_guidance_schedule", [&]() { t->t.g_sched.assign(scales_host, scales_host + count); return 0; });
}
int ladi_tryon_set_ip_adapter(ladi_tryon* t, const void* embeds, const void* negative_embeds) {
    if (!t) { set_error("ladi_tryon_set_ip_adapter: null handle"); return -1; }
    t->t.ip_pos = reinterpret_cast<const h16*>(embeds);
    t->t.ip_neg = embeds ? reinterpret_cast<const h16*>(negative_embeds) : nullptr;
    t->t.ip_T = 0;
    return 0;
}
int ladi_tryon_set_ip_adapter_seq(ladi_tryon* t, const void* hidden, const void* negative_hidden, int T) {
    if (!t) { set_error("ladi_tryon_set_ip_adapter_seq: null handle"); return -1; }
    if (hidden && T < 1) { set_error("ladi_tryon_set_ip_adapter_seq: T = " + std::to_string(T) + ", hidden states have at least one token"); return -1; }
    t->t.ip_pos = reinterpret_cast<const h16*>(hidden);
    t->t.ip_neg = hidden ? reinterpret_cast<const h16*>(negative_hidden) : nullptr;
    t->t.ip_T = hidden ? T : 0;
    return 0;
}
int ladi_tryon_set_pag(ladi_tryon* t, const float* scales_host, int count) {
    if (!t || count < 0) { set_error("ladi_tryon_set_pag: null handle or negative count"); return -1; }
    if (!scales_host || count == 0) { t->t.pag_sched.clear(); return 0; }
    for (int i = 0; i < count; ++i)
        if (!std::isfinite(scales_host[i]) || scales_host[i] < 0.f) {
            set_error("ladi_tryon_set_pag: entry " + std::to_string(i) + " is negative or not finite");
            return -1;
        }
    return guarded("ladi_tryon_set_pag", [&]() { t->t.pag_sched.assign(scales_host, scales_host + count); return 0; });
}
int ladi_tryon_set_guidance_rescale(ladi_tryon* t, float phi) {
    if (!t || !(phi >= 0.f && phi <= 1.f)) { set_error("ladi_tryon_set_guidance_rescale: null handle, or phi outside [0, 1]"); return -1; }
    t->t.phi = phi;
    return 0;
}
int ladi_tryon_cond_only_evals(ladi_tryon* t) { return t ? t->t.last_cond_only : -1; }
int ladi_tryon_plan_forms(int evals, int first_step, int steps, float guidance, const float* guidance_tab_host, int guidance_count, float phi,
                          const float* pag_tab_host, int pag_count, const unsigned char* full_flags_host, int flag_count, unsigned char* forms_out) {
    if (evals < 1 || guidance_count < 0 || pag_count < 0 || flag_count < 0 || !forms_out) {
        set_error("ladi_tryon_plan_forms: evals < 1, a negative count or no output");
        return -1;
    }
    return guarded("ladi_tryon_plan_forms", [&]() {
        EvalPlan p;
        const std::vector<float> g(guidance_tab_host, guidance_tab_host + (guidance_tab_host ? guidance_count : 0));
        const std::vector<float> pag(pag_tab_host, pag_tab_host + (pag_tab_host ? pag_count : 0));
        const std::vector<unsigned char> fc(full_flags_host, full_flags_host + (full_flags_host ? flag_count : 0));
        if (plan_evals(p, evals, first_step, steps, guidance, g, phi, pag, fc)) { set_error(p.error); return p.rc; }
        std::memcpy(forms_out, p.form.data(), (size_t)evals);
        return evals;
    });
}
long long ladi_tryon_graph_captures(ladi_tryon* t) { return t ? t->t.graphs.captures : -1; }
int ladi_tryon_set_sag(ladi_tryon* t, float sag_scale) {
    if (!t || !std::isfinite(sag_scale) || sag_scale < 0.f) { set_error("ladi_tryon_set_sag: null handle, or a negative or non-finite scale"); return -1; }
    t->t.sag_scale = sag_scale;
    return 0;
}
int ladi_tryon_plan_forms_sag(int evals, int first_step, int steps, float guidance, const float* guidance_tab_host, int guidance_count, float phi,
                              const float* pag_tab_host, int pag_count, const unsigned char* full_flags_host, int flag_count, float sag_scale,
                              int scheduler, int lat_h, int lat_w, int tome_mid_merges, unsigned char* forms_out) {
    if (evals < 1 || guidance_count < 0 || pag_count < 0 || flag_count < 0 || !forms_out || !std::isfinite(sag_scale) || sag_scale < 0.f) {
        set_error("ladi_tryon_plan_forms_sag: evals < 1, a negative count, no output, or a negative or non-finite SAG scale");
        return -1;
    }
    return guarded("ladi_tryon_plan_forms_sag", [&]() {
        EvalPlan p;
        const std::vector<float> g(guidance_tab_host, guidance_tab_host + (guidance_tab_host ? guidance_count : 0));
        const std::vector<float> pag(pag_tab_host, pag_tab_host + (pag_tab_host ? pag_count : 0));
        const std::vector<unsigned char> fc(full_flags_host, full_flags_host + (full_flags_host ? flag_count : 0));
        SagPlan sp; sp.scale = sag_scale; sp.scheduler = scheduler; sp.h = lat_h; sp.w = lat_w; sp.mid_merges = tome_mid_merges != 0;
        if (plan_evals(p, evals, first_step, steps, guidance, g, phi, pag, fc, &sp)) { set_error(p.error); return p.rc; }
        std::memcpy(forms_out, p.form.data(), (size_t)evals);
        return evals;
    });
}
int ladi_tryon_set_feature_cache(ladi_tryon* t, const unsigned char* full_flags_host, int count, int branch) {
    if (!t || count < 0) { set_error("ladi_tryon_set_feature_cache: null handle or negative count"); return -1; }
    if (!full_flags_host || count == 0) { t->t.fc_plan.clear(); t->t.fc_branch = 0; return 0; }
    if (branch < 0 || branch > 2) { set_error("ladi_tryon_set_feature_cache: branch " + std::to_string(branch) + " out of range [0, 2]"); return -2; }
    return guarded("ladi_tryon_set_feature_cache", [&]() {
        t->t.fc_plan.assign(full_flags_host, full_flags_host + count);
        t->t.fc_branch = branch;
        return 0;
    });
}
int ladi_tryon_set_preserve(ladi_tryon* t, int mode_bits, float feather_sigma) {
    if (mode_bits < 0 || mode_bits > 3) { set_error("ladi_tryon_set_preserve: mode bits " + std::to_string(mode_bits) + " outside 0 .. 3 (bit 0 latents, bit 1 pixels)"); return -1; }
    if (!(feather_sigma >= 0.f) || !(feather_sigma <= 32.f)) {
        set_error("ladi_tryon_set_preserve: feather sigma " + std::to_string(feather_sigma) + " outside [0, 32]");
        return -1;
    }
    if (feather_sigma > 0.f && !(mode_bits & 2)) { set_error("ladi_tryon_set_preserve: a feather needs the pixels mode (bit 1)"); return -1; }
    if (!t) { set_error("ladi_tryon_set_preserve: null handle"); return -1; }
    t->t.preserve_mode = mode_bits; t->t.preserve_sigma = feather_sigma;
    return 0;
}
int ladi_tryon_shallow_evals(ladi_tryon* t) { return t ? t->t.last_shallow : -1; }
int ladi_tryon_set_step_callback(ladi_tryon* t, ladi_step_callback fn, void* user, int every, float* latents_nchw_dev) {
    if (!t) { set_error("ladi_tryon_set_step_callback: null handle"); return -1; }
    if (fn && (every < 1 || !latents_nchw_dev)) { set_error("ladi_tryon_set_step_callback: every must be >= 1 and the latents buffer set"); return -1; }
    t->t.cb_fn = fn; t->t.cb_user = fn ? user : nullptr; t->t.cb_every = fn ? every : 1; t->t.cb_latents = fn ? latents_nchw_dev : nullptr;
    return 0;
}
int ladi_tryon_set_trace(ladi_tryon* t, float* eps_trace, float* latents_trace, int cap_evals) {
    if (!t || cap_evals < 0) return -1;
    t->t.trace_eps = eps_trace; t->t.trace_lat = latents_trace; t->t.trace_cap = (eps_trace || latents_trace) ? cap_evals : 0;
    return 0;
}

// ------------------------------------------------------------------------------------------------ range probe
ladi_probe* ladi_probe_create(int max_points) {
    ladi_probe* h = nullptr;
    int rc = guarded("ladi_probe_create", [&]() { require_gpu(); h = new ladi_probe(max_points); return 0; });
    return rc ? nullptr : h;
}
void ladi_probe_destroy(ladi_probe* p) {
    if (!p) return;
    {
        std::lock_guard<std::mutex> lk(g_probe_mu);
        auto it = g_probe_refs.find(&p->p);
        if (it != g_probe_refs.end() && it->second > 0) {
            // a module would go on launching into the freed slots: keep the probe (a leak, not a dangling pointer) and say so
            set_error("ladi_probe_destroy: the probe is still attached to " + std::to_string(it->second) + " module(s); nothing was destroyed -- detach (attach NULL) or destroy the modules first");
            return;
        }
        g_probe_refs.erase(&p->p);
    }
    delete p;
}
int ladi_unet_attach_probe(ladi_unet* u, ladi_probe* p) {
    if (!u) { set_error("ladi_unet_attach_probe: null handle"); return -1; }
    set_module_probe(u->u.probe, p);
    return 0;
}
int ladi_vae_attach_probe(ladi_vae* v, ladi_probe* p) {
    if (!v) { set_error("ladi_vae_attach_probe: null handle"); return -1; }
    set_module_probe(v->v.probe, p);
    return 0;
}
int ladi_emasc_attach_probe(ladi_emasc* e, ladi_probe* p) {
    if (!e) { set_error("ladi_emasc_attach_probe: null handle"); return -1; }
    set_module_probe(e->e.probe, p);
    return 0;
}
int ladi_probe_count(const ladi_probe* p) { return p ? (int)p->p.names.size() : -1; }
const char* ladi_probe_name(const ladi_probe* p, int i) { return (p && i >= 0 && i < (int)p->p.names.size()) ? p->p.names[i].c_str() : nullptr; }
int ladi_probe_read(ladi_probe* p, float* absmax_out, unsigned* nonfinite_out, int cap, void* stream) {
    return guarded("ladi_probe_read", [&]() {
        if (!p || cap < 0) throw std::runtime_error("null handle or negative cap");
        p->p.read(absmax_out, nonfinite_out, cap, S(stream));
        return (int)p->p.names.size();
    });
}
int ladi_probe_read_rank(ladi_probe* p, unsigned* rank_out, int cap, void* stream) {
    return guarded("ladi_probe_read_rank", [&]() {
        if (!p || !rank_out || cap < 0) throw std::runtime_error("null argument or negative cap");
        p->p.read_rank(rank_out, cap, S(stream));
        return (int)p->p.names.size();
    });
}
int ladi_probe_reset(ladi_probe* p, void* stream) {
    return guarded("ladi_probe_reset", [&]() {
        if (!p) throw std::runtime_error("null handle");
        p->p.reset(S(stream));
        return 0;
    });
}
int ladi_op_absmax(const void* x, int rows, int C, int ld, float* absmax_dev, unsigned* nonfinite_dev, void* stream) {
    return guarded("ladi_op_absmax", [&]() {
        int rc = ladi_launch_absmax_probe(reinterpret_cast<const h16*>(x), rows, C, ld, reinterpret_cast<unsigned*>(absmax_dev), nonfinite_dev, S(stream));
        if (rc) set_error("ladi_op_absmax: bad arguments (rows >= 0, C >= 1, ld >= C, non-null pointers) rc=" + std::to_string(rc));
        return rc;
    });
}

void ladi_igemm_set_autotune(int on) { ladi_igemm_autotune(on); }
void ladi_igemm_set_splitk_two_pass(int on) { ladi_igemm_splitk_two_pass(on); }
void ladi_profile_igemm_enable(int on) { ladi_igemm_profile_enable(on); }
int ladi_profile_igemm_collect(double* out, int n_out) { return ladi_igemm_profile_collect(out, n_out); }
int ladi_profile_igemm_symbols(char* buf, int n) { return ladi_igemm_profile_symbols(buf, n); }
int ladi_igemm_cfg_count(void) { return ladi_igemm_num_cfgs(); }
int ladi_igemm_last_launch(int out[4]) {
    if (!out) return -1;
    ladi_igemm_last_launch_info(out);
    return 0;
}
const char* ladi_igemm_cfg_symbol_name(int cfg) { return ladi_igemm_cfg_symbol(cfg); }
int ladi_igemm_tune_key(const ladi_igemm_desc* d, int batch, int key[8]) {
    if (!d || !key) return -100;
    IGemmArgs a;
    std::memcpy(&a, d, sizeof(a));
    return ladi_igemm_key_of(a, batch, key);
}
int ladi_igemm_tune_lookup(const int key[8]) { return key ? ladi_igemm_tuned_lookup(key) : 0; }
int ladi_igemm_tune_put(const int key[8], int cfg) { return key ? ladi_igemm_tuned_put(key, cfg) : -1; }
int ladi_igemm_cfg_admissible(const ladi_igemm_desc* d, int batch, int cfg, int strict) {
    if (!d) return 0;
    IGemmArgs a;
    std::memcpy(&a, d, sizeof(a));
    return ladi_igemm_admissible(a, batch, cfg, strict);
}
int ladi_igemm_last_selection(int out[2]) {
    if (!out) return -1;
    ladi_igemm_selection(out);
    return 0;
}
void ladi_igemm_launch_log(int on) { ladi_igemm_log_enable(on); }
int ladi_igemm_launch_log_read(char* buf, int n) { return ladi_igemm_log_read(buf, n); }

// ------------------------------------------------------------------------------------------------ op level
int ladi_op_igemm(const ladi_igemm_desc* d, int batch, int tile_cfg, void* stream) {
    return guarded("ladi_op_igemm", [&]() {
        IGemmArgs a;
        std::memcpy(&a, d, sizeof(a));
        int rc = ladi_launch_igemm(a, batch, tile_cfg, S(stream));
        if (rc) set_error("igemm launch rc=" + std::to_string(rc) + (rc == -20 ? std::string(": ") + ladi_igemm_span_refusal() : std::string()));
        return rc;
    });
}
// the runtime's group_norm() (runtime_core.cpp) on views of the caller's dense tensors: the form every model runs for the same operands
int ladi_op_group_norm(const void* src0, int C0, const void* src1, int C1, int n, int HW, int groups, const void* gamma, const void* beta,
                       float eps, int silu, const void* add, void* out, float* stats, void* stream) {
    return guarded("ladi_op_group_norm", [&]() {
        hipStream_t st = S(stream);
        (void)stats;  // legacy scratch argument (unused: statistics are atomics-free partial rows in a per-stream arena now)
        const Act x = op_view(src0, n, HW, C0), x2 = op_view(src1, n, HW, C1), ad = op_view(add, n, HW, C0 + C1), o = op_view(out, n, HW, C0 + C1);
        DNorm nm; nm.g = reinterpret_cast<h16*>(const_cast<void*>(gamma)); nm.b = reinterpret_cast<h16*>(const_cast<void*>(beta)); nm.c = C0 + C1;
        std::lock_guard<std::mutex> lk(g_op_mu);
        run_planned(op_arena(st), st, [&](Ctx& c) { (void)group_norm(c, nm, x, C1 ? &x2 : nullptr, groups, eps, silu, add ? &ad : nullptr, &o); });
        return 0;
    });
}
// ladi_op_igemm that also reports the pixels per row of the statistics the launch wrote into d->stats (0: it wrote none)
int ladi_op_igemm_stats(const ladi_igemm_desc* d, int batch, int tile_cfg, int* stats_row_px, void* stream) {
    return guarded("ladi_op_igemm_stats", [&]() {
        IGemmArgs a;
        std::memcpy(&a, d, sizeof(a));
        int rc = ladi_launch_igemm(a, batch, tile_cfg, S(stream), stats_row_px);
        if (rc) set_error("igemm launch rc=" + std::to_string(rc) + (rc == -20 ? std::string(": ") + ladi_igemm_span_refusal() : std::string()));
        return rc;
    });
}
// ladi_op_group_norm on sources that bring their producers' partial rows (Act::st_part / st_px): the runtime's own dispatch over gn_norm,
// gn_reduce + gn_norm and gn_finalize + gn_apply, on rows the caller placed
int ladi_op_group_norm_rows(const void* src0, int C0, const float* part0, int px0, const void* src1, int C1, const float* part1, int px1, int n,
                            int HW, int groups, const void* gamma, const void* beta, float eps, int silu, const void* add, void* out, void* stream) {
    return guarded("ladi_op_group_norm_rows", [&]() {
        hipStream_t st = S(stream);
        if (n < 1 || HW < 1 || px0 < 0 || px1 < 0 || (px0 > 0 && (!part0 || HW % px0)) || (C1 && px1 > 0 && (!part1 || HW % px1)))
            throw std::runtime_error("rows of px pixels need a buffer and HW % px == 0");
        Act x = op_view(src0, n, HW, C0), x2 = op_view(src1, n, HW, C1);
        const Act ad = op_view(add, n, HW, C0 + C1), o = op_view(out, n, HW, C0 + C1);
        if (px0 > 0) { x.st_part = const_cast<float*>(part0); x.st_px = px0; }
        if (C1 && px1 > 0) { x2.st_part = const_cast<float*>(part1); x2.st_px = px1; }
        DNorm nm; nm.g = reinterpret_cast<h16*>(const_cast<void*>(gamma)); nm.b = reinterpret_cast<h16*>(const_cast<void*>(beta)); nm.c = C0 + C1;
        std::lock_guard<std::mutex> lk(g_op_mu);
        run_planned(op_arena(st), st, [&](Ctx& c) { (void)group_norm(c, nm, x, C1 ? &x2 : nullptr, groups, eps, silu, add ? &ad : nullptr, &o); });
        return 0;
    });
}
// fused transformer sub-blocks of the C = 320 level from plain operands: the packings the kernels read are built here, per call (op-level
// entry points are for tests; the UNet packs once at load / per context)
int ladi_op_xattn_block(const void* x, const void* ln_gamma, const void* ln_beta, float eps, const void* wq, const void* kv, int L, const void* wo,
                        const void* bo, int n, int T, void* out, void* stream) {
    return guarded("ladi_op_xattn_block", [&]() {
        hipStream_t st = S(stream);
        if (!ladi_xf_fused_eligible(320, 5, T, L) || n < 1) throw std::runtime_error("unsupported shape (C = 320, 5 heads, T % 128 == 0, L <= 96)");
        h16* buf = nullptr;
        const size_t nk = ladi_xf_kp_elems(n), nv = ladi_xf_vt_elems(n), nw = ladi_xf_wo_packed_elems();
        HIP_OK(hipMalloc(reinterpret_cast<void**>(&buf), (nk + nv + nw) * sizeof(h16)));
        int rc = ladi_launch_pack_kv_tiles((const h16*)kv, n, L, 320, buf, buf + nk, st);
        if (!rc) rc = ladi_launch_pack_wo((const h16*)wo, buf + nk + nv, st);
        XAttnBlockArgs a;
        a.x = (const h16*)x; a.ln_g = (const h16*)ln_gamma; a.ln_b = (const h16*)ln_beta; a.ln_eps = eps; a.Wq = (const h16*)wq;
        a.Kp = buf; a.Vt = buf + nk; a.Wo = buf + nk + nv; a.bo = (const h16*)bo; a.res = (const h16*)x; a.out = (h16*)out;
        a.P = n * T; a.T = T; a.nk = L; a.scale = 0.125f;
        if (!rc) rc = ladi_launch_xattn_block(a, st);
        HIP_OK(hipStreamSynchronize(st));
        (void)hipFree(buf);
        if (rc) set_error("xattn_block rc=" + std::to_string(rc));
        return rc;
    });
}
int ladi_op_ff_block(const void* x, const void* ln_gamma, const void* ln_beta, float eps, const void* w1_geglu, const void* b1_geglu, const void* w2,
                     const void* bo, int P, void* out, void* stream) {
    return guarded("ladi_op_ff_block", [&]() {
        hipStream_t st = S(stream);
        h16* buf = nullptr;
        HIP_OK(hipMalloc(reinterpret_cast<void**>(&buf), ladi_xf_w2_packed_elems() * sizeof(h16)));
        int rc = ladi_launch_pack_w2((const h16*)w2, buf, st);
        FFBlockArgs a;
        a.x = (const h16*)x; a.ln_g = (const h16*)ln_gamma; a.ln_b = (const h16*)ln_beta; a.ln_eps = eps;
        a.W1 = (const h16*)w1_geglu; a.b1 = (const h16*)b1_geglu; a.W2 = buf; a.bo = (const h16*)bo; a.res = (const h16*)x; a.out = (h16*)out; a.P = P;
        if (!rc) rc = ladi_launch_ff_block(a, st);
        HIP_OK(hipStreamSynchronize(st));
        (void)hipFree(buf);
        if (rc) set_error("ff_block rc=" + std::to_string(rc));
        return rc;
    });
}
int ladi_op_layer_norm(const void* x, const void* gamma, const void* beta, float eps, int rows, int C, void* out, void* stream) {
    return ladi_launch_layernorm((const h16*)x, C, (const h16*)gamma, (const h16*)beta, eps, rows, C, (h16*)out, C, S(stream));
}
int ladi_op_layer_norm_ld(const void* x, int ldx, const void* gamma, const void* beta, float eps, int rows, int C, void* out, int ldo, void* stream) {
    return ladi_launch_layernorm((const h16*)x, ldx, (const h16*)gamma, (const h16*)beta, eps, rows, C, (h16*)out, ldo, S(stream));
}
// rc -3 of the flash kernel: the keys of one sample span more than its 32-bit K / V offsets reach (attention.hip ladi_launch_flash_attn64)
static int flash_attn_rc(const char* what, const AttnArgs& a, int rc) {
    if (rc == -3)
        set_error(std::string(what) + ": refused: Nk = " + std::to_string(a.Nk) + " keys at row strides ldk = " + std::to_string(a.ldk) + ", ldv = " +
                  std::to_string(a.ldv) + " span " + std::to_string(2 * ((long long)(a.Nk - 1) * std::max(a.ldk, a.ldv) + 64)) +
                  " bytes per sample; the K / V stream reaches less than 2147483647");
    return rc;
}
int ladi_op_attention(const void* q, const void* k, const void* v, void* o, int ldq, int ldk, int ldv, int ldo, long long sq, long long sk,
                      long long sv, long long so, int n, int heads, int Nq, int Nk, float scale, void* stream) {
    AttnArgs a;
    a.q = (const h16*)q; a.k = (const h16*)k; a.v = (const h16*)v; a.o = (h16*)o;
    a.ldq = ldq; a.ldk = ldk; a.ldv = ldv; a.ldo = ldo; a.sq = sq; a.sk = sk; a.sv = sv; a.so = so;
    a.n = n; a.heads = heads; a.Nq = Nq; a.Nk = Nk; a.scale = scale;
    return flash_attn_rc("ladi_op_attention", a, ladi_launch_flash_attn64(a, S(stream)));
}
int ladi_op_attention_causal(const void* q, const void* k, const void* v, void* o, int ldq, int ldk, int ldv, int ldo, long long sq,
                             long long sk, long long sv, long long so, int n, int heads, int Nq, int Nk, float scale, int causal,
                             void* stream) {
    if (causal && Nq != Nk) return -1;
    AttnArgs a;
    a.q = (const h16*)q; a.k = (const h16*)k; a.v = (const h16*)v; a.o = (h16*)o;
    a.ldq = ldq; a.ldk = ldk; a.ldv = ldv; a.ldo = ldo; a.sq = sq; a.sk = sk; a.sv = sv; a.so = so;
    a.n = n; a.heads = heads; a.Nq = Nq; a.Nk = Nk; a.scale = scale; a.causal = causal ? 1 : 0;
    return flash_attn_rc("ladi_op_attention_causal", a, ladi_launch_flash_attn64(a, S(stream)));
}
int ladi_op_attention_generic(const void* q, const void* k, const void* v, void* o, int ldq, int ldk, int ldv, int ldo, long long sq,
                              long long sk, long long sv, long long so, int n, int heads, int head_dim, int Nq, int Nk, float scale,
                              void* stream) {
    AttnArgs a;
    a.q = (const h16*)q; a.k = (const h16*)k; a.v = (const h16*)v; a.o = (h16*)o;
    a.ldq = ldq; a.ldk = ldk; a.ldv = ldv; a.ldo = ldo; a.sq = sq; a.sk = sk; a.sv = sv; a.so = so;
    a.n = n; a.heads = heads; a.Nq = Nq; a.Nk = Nk; a.scale = scale;
    return ladi_launch_attn_generic(a, head_dim, S(stream));
}
int ladi_op_attention_wide(const void* q, const void* k, const void* vt, void* o, int ldq, int ldk, int ldvt, int ldo, long long sq, long long sk,
                           long long svt, long long so, int n, int head_dim, int Nq, int Nk, float scale, void* stream) {
    AttnArgs a;
    a.q = (const h16*)q; a.k = (const h16*)k; a.v = (const h16*)vt; a.o = (h16*)o;
    a.ldq = ldq; a.ldk = ldk; a.ldv = ldvt; a.ldo = ldo; a.sq = sq; a.sk = sk; a.sv = svt; a.so = so;
    a.n = n; a.heads = 1; a.Nq = Nq; a.Nk = Nk; a.scale = scale;
    return ladi_launch_attn_wide(a, head_dim, S(stream));
}
int ladi_op_resize_bilinear_aa(const void* src, int dtype, int planes, int H, int W, void* dst, int out_dtype, int Ho, int Wo, void* stream) {
    return ladi_launch_resize_bilinear_aa(src, dtype == LADI_F32, planes, H, W, dst, out_dtype == LADI_F32, Ho, Wo, S(stream));
}
int ladi_clock_probe(unsigned long long wall_ticks_100mhz, unsigned long long* out2_dev, void* stream) {
    if (!out2_dev || wall_ticks_100mhz == 0 || wall_ticks_100mhz > 100000000ull) return -1;      // at most one second
    return ladi_launch_clock_probe(wall_ticks_100mhz, out2_dev, S(stream));
}
int ladi_op_clip_preprocess(const void* src, int dtype, int B, int H, int W, int size, const float* mean3, const float* std3, void* dst_f16, void* stream) {
    if (!src || !dst_f16 || !mean3 || !std3 || B <= 0 || size <= 0) return -1;
    ResizeEpi e; e.on = 1; e.C = 3; e.pre_mul = 0.5f; e.pre_add = 0.5f; e.quant = 255.f;   // the processor's uint8 round trip (elementwise.hip)
    for (int i = 0; i < 3; ++i) { e.sub[i] = mean3[i]; e.div[i] = std3[i]; }
    e.sub[3] = 0.f; e.div[3] = 1.f;
    return ladi_launch_resize_bilinear_aa(src, dtype == LADI_F32, B * 3, H, W, dst_f16, 0, size, size, S(stream), &e);
}
int ladi_op_grid_sample_border(const void* src, int dtype, int B, int C, int H, int W, const float* grid, int Ho, int Wo, void* dst,
                               int out_dtype, void* stream) {
    return ladi_launch_grid_sample_border(src, dtype == LADI_F32, B, C, H, W, grid, Ho, Wo, dst, out_dtype == LADI_F32, S(stream));
}
int ladi_op_maxpool2(const void* src, int n, int H, int W, int C, void* dst, void* stream) {
    return ladi_launch_maxpool2((const h16*)src, C, n, H, W, C, (h16*)dst, C, S(stream));
}
int ladi_op_upsample2x_bilinear(const void* src, int n, int H, int W, int C, void* dst, void* stream) {
    return ladi_launch_upsample2x_bilinear_ac((const h16*)src, C, n, H, W, C, (h16*)dst, C, S(stream));
}
int ladi_op_softmax_rows(const float* Sm, int rows, int cols, float scale, void* P, void* stream) {
    return ladi_launch_softmax_rows(Sm, rows, cols, scale, (h16*)P, S(stream));
}
int ladi_op_small_linear(const void* x, int x_f32, int ldx, const void* W, const void* bias, const void* res, int ldr, int M, int N, int K,
                         int act, int pre_silu, void* out, int out_f32, int ldo, void* stream) {
    return ladi_launch_small_linear(x, x_f32, ldx, (const h16*)W, (const h16*)bias, (const h16*)res, ldr, M, N, K, act, pre_silu, out,
                                    out_f32, ldo, S(stream));
}
int ladi_op_nchw_to_nhwc(const void* src, int dtype, int n, int C, int H, int W, void* dst, int ld, void* stream) {
    return ladi_launch_nchw_to_nhwc(src, dtype == LADI_F32, n, C, H, W, (h16*)dst, ld, S(stream));
}
int ladi_op_nhwc_to_nchw(const void* src, int ld, int n, int C, int H, int W, void* dst, int dtype, void* stream) {
    return ladi_launch_nhwc_to_nchw((const h16*)src, ld, n, C, H, W, dst, dtype == LADI_F32, S(stream));
}
int ladi_op_prepare_mask(const void* image, const void* mask, int dtype, int B, int H, int W, void* masked, int ld, void* mask_bin, void* stream) {
    return ladi_launch_prepare_mask(image, dtype == LADI_F32, mask, dtype == LADI_F32, B, H, W, (h16*)masked, ld, (h16*)mask_bin, S(stream));
}
int ladi_op_mask_down(const void* mask, int B, int H, int W, int s, void* out, void* stream) {
    if (s <= 0 || H % s || W % s) return -1;
    return ladi_launch_mask_down((const h16*)mask, B, H, W, s, (h16*)out, S(stream));
}
int ladi_op_pose_down8(const void* pose, int dtype, int B, int C, int H, int W, void* out, void* stream) {
    if (H % 8 || W % 8) return -1;
    return ladi_launch_pose_down8(pose, dtype == LADI_F32, B, C, H, W, (h16*)out, S(stream));
}
int ladi_op_posterior_sample(const void* moments, int ldm, const float* noise, int B, int hw, float scaling, float* lat, void* stream) {
    return ladi_launch_posterior_sample((const h16*)moments, ldm, noise, B, hw, scaling, lat, S(stream));
}
int ladi_op_assemble_input(void* unet_in, int ld, int B, int hw, int cfg, const float* latents, const void* mask_lat, const float* masked_lat,
                           const void* pose, int pose_ch, const float* cloth_lat, void* stream) {
    return ladi_launch_assemble_static((h16*)unet_in, ld, B, hw, cfg, latents, (const h16*)mask_lat, masked_lat, (const h16*)pose, pose_ch,
                                       cloth_lat, cloth_lat ? 1 : 0, 1.0f, S(stream));
}
// helper kernels on their own (tests/test_gpu_helpers.py): cast, launch, return the launcher's code
int ladi_op_attention_single_query(const void* q, int ldq, const void* k, int ldk, const void* v, int ldv, void* o, int ldo, int n, int heads,
                                   int d, int Nk, long long sk, long long sv, float scale, void* stream) {
    return ladi_launch_attn_single_query((const h16*)q, ldq, (const h16*)k, ldk, (const h16*)v, ldv, (h16*)o, ldo, n, heads, d, Nk, sk, sv, scale,
                                         S(stream));
}
int ladi_op_conv_f32(const ladi_conv_f32_desc* d, int batch, void* stream) {
    if (!d) return -1;
    ConvF32Args a;
    std::memcpy(&a, d, sizeof(a));
    return ladi_launch_conv_f32(a, batch, S(stream));
}
int ladi_op_nchw_to_nhwc_f32(const void* src, int dtype, int n, int C, int H, int W, float* dst, int ld, void* stream) {
    return ladi_launch_nchw_to_nhwc_f32(src, dtype == LADI_F32, n, C, H, W, dst, ld, S(stream));
}
int ladi_op_nhwc_to_nchw_f32(const float* src, int ld, int n, int C, int H, int W, void* dst, int dtype, void* stream) {
    return ladi_launch_nhwc_to_nchw_f32(src, ld, n, C, H, W, dst, dtype == LADI_F32, S(stream));
}
int ladi_op_channel_affine_f32(float* x, int ld, long long n_pix, int C, const float* scale, const float* shift, void* stream) {
    return ladi_launch_channel_affine_f32(x, ld, (size_t)n_pix, C, scale, shift, S(stream));
}
int ladi_op_l2norm_rows_f32(float* x, int ld, int rows, int C, void* stream) { return ladi_launch_l2norm_rows_f32(x, ld, rows, C, S(stream)); }
int ladi_op_gather_rows_f32(const float* src, const int* rows, int n, int H, float* dst, void* stream) {
    return ladi_launch_gather_rows_f32(src, rows, n, H, dst, S(stream));
}
int ladi_op_maxpool2_f32(const float* src, int lds, int n, int H, int W, int C, float* dst, int ldd, void* stream) {
    return ladi_launch_maxpool2_f32(src, lds, n, H, W, C, dst, ldd, S(stream));
}
int ladi_op_upsample2x_bilinear_f32(const float* src, int lds, int n, int H, int W, int C, float* dst, int ldd, void* stream) {
    return ladi_launch_upsample2x_bilinear_ac_f32(src, lds, n, H, W, C, dst, ldd, S(stream));
}
int ladi_op_linear_f32(const float* x, int ldx, const float* W, const float* b, int M, int N, int K, int act, float* out, int ldo, void* stream) {
    return ladi_launch_linear_f32(x, ldx, W, b, M, N, K, act, out, ldo, S(stream));
}
int ladi_op_channel_affine(const void* x, int ldx, long long n_pix, int C, const float* scale, const float* shift, void* y, int ldy, void* stream) {
    return ladi_launch_channel_affine((const h16*)x, ldx, (size_t)n_pix, C, scale, shift, (h16*)y, ldy, S(stream));
}
int ladi_op_l2norm_rows(const void* x, int ldx, int rows, int C, void* y, int ldy, void* stream) {
    return ladi_launch_l2norm_rows((const h16*)x, ldx, rows, C, (h16*)y, ldy, S(stream));
}
int ladi_op_gather_rows(const void* src, const int* rows, int n, int H, void* dst, void* stream) {
    return ladi_launch_gather_rows((const h16*)src, rows, n, H, (h16*)dst, S(stream));
}
int ladi_op_tps_grid(const float* coor, const float* inv, const float* ctrl, int N, int B, int H, int W, float* grid, void* stream) {
    return ladi_launch_tps_grid(coor, inv, ctrl, N, B, H, W, grid, S(stream));
}
int ladi_op_text_meta(const int* ids, int B, int T, int vstar, int use_words, int* first, int* eot, void* stream) {
    return ladi_launch_text_meta(ids, B, T, vstar, use_words, first, eot, S(stream));
}
int ladi_op_text_embed(const int* ids, const int* first, int nv, const void* tok, const void* pos, const void* wemb, int B, int T, int H,
                       int vocab, void* out, void* stream) {
    return ladi_launch_text_embed(ids, first, nv, (const h16*)tok, (const h16*)pos, (const h16*)wemb, B, T, H, vocab, (h16*)out, S(stream));
}
int ladi_op_patchify(const void* px, int dtype, int B, int S_, int ps, int KP, void* out, void* stream) {
    return ladi_launch_patchify(px, dtype == LADI_F32, B, S_, ps, KP, (h16*)out, S(stream));
}
int ladi_op_timestep_embedding(const float* t, int count, int dim, float* out, void* stream) {
    return ladi_launch_timestep_embedding(t, count, dim, out, S(stream));
}
int ladi_op_image_post(const void* src, int ld, int n_pix, void* dst, int dst_u8, void* stream) {
    return ladi_launch_image_post((const h16*)src, ld, n_pix, dst, dst_u8, S(stream));
}
int ladi_op_post_quant(const float* lat, const float* pq, float inv_sf, int n, void* dst, int ld, void* stream) {
    return ladi_launch_post_quant(lat, pq, inv_sf, n, (h16*)dst, ld, S(stream));
}
int ladi_op_lat_nchw_to_pix(const float* src, int B, int hw, float scale, float* dst, void* stream) {
    return ladi_launch_lat_nchw_to_pix(src, B, hw, scale, dst, S(stream));
}
int ladi_op_init_latents(const float* init, int hs, int ws, const float* noise, int B, int h, int w, float k_x, float k_n, float* out, void* stream) {
    return guarded("ladi_op_init_latents", [&]() {
        if (!init || !out) throw std::runtime_error("null init or out");
        if (hs < 1 || ws < 1 || B < 1 || h < 1 || w < 1) throw std::runtime_error("every size has to be >= 1");
        if (!noise && k_n != 0.f) throw std::runtime_error("null noise with k_n != 0");
        const int rc = ladi_launch_init_latents(init, hs, ws, noise, B, h, w, k_x, k_n, out, S(stream));
        if (rc) throw std::runtime_error("launch refused (sizes too large) or failed");
        return 0;
    });
}
int ladi_op_lat_pix_to_nchw(const float* src, int B, int hw, float* dst, void* stream) { return ladi_launch_lat_pix_to_nchw(src, B, hw, dst, S(stream)); }
int ladi_op_latents_import(const float* src, int B, int hw, float* latents, void* unet_in, int ld_in, int cfg, float in_scale, void* stream) {
    return ladi_launch_latents_import(src, B, hw, latents, (h16*)unet_in, ld_in, cfg, in_scale, S(stream));
}
int ladi_op_scale_h16(const void* src, int lds, void* dst, int ldd, long long n_pix, int C, float s, void* stream) {
    return ladi_launch_scale_h16((const h16*)src, lds, (h16*)dst, ldd, (size_t)n_pix, C, s, S(stream));
}
int ladi_op_fill_f32(float* p, long long n, float v, void* stream) { return ladi_launch_fill_f32(p, (size_t)n, v, S(stream)); }
int ladi_op_freeu(void* hidden, int ld_h, int C_h, float b, const void* skip, int ld_s, int C_s, float s, void* skip_out, int ld_d, int n, int H,
                  int W, void* stream) {
    return guarded("ladi_op_freeu", [&]() {
        if (!hidden && !skip) throw std::runtime_error("hidden and skip are both null");
        if (n < 1 || H < 1 || W < 1) throw std::runtime_error("every size has to be >= 1");
        if (hidden && (C_h < 16 || (C_h & 15))) throw std::runtime_error("C_h = " + std::to_string(C_h) + " is not a multiple of 16");
        if (skip && (C_s < 8 || (C_s & 7))) throw std::runtime_error("C_s = " + std::to_string(C_s) + " is not a multiple of 8");
        if (skip && !skip_out) throw std::runtime_error("skip without skip_out");
        if ((hidden && (ld_h < C_h || (ld_h & 7) || ((uintptr_t)hidden & 15))) ||
            (skip && (ld_s < C_s || ld_d < C_s || (ld_s & 7) || (ld_d & 7) || ((uintptr_t)skip & 15) || ((uintptr_t)skip_out & 15))))
            throw std::runtime_error("every row stride has to be a multiple of 8 and >= its channel count, every pointer 16-byte aligned");
        const int rc = ladi_launch_freeu(reinterpret_cast<h16*>(hidden), ld_h, C_h, b, reinterpret_cast<const h16*>(skip), ld_s, C_s, s,
                                         reinterpret_cast<h16*>(skip_out), ld_d, n, H, W, S(stream));
        if (rc) throw std::runtime_error("launch refused or failed (rc = " + std::to_string(rc) + ")");
        return 0;
    });
}
int ladi_op_pag_identity(const void* v, int ldv, void* o, int ldo, long long rows, int C, void* stream) {
    return guarded("ladi_op_pag_identity", [&]() {
        if (!v || !o) throw std::runtime_error("null v or o");
        if (rows < 1) throw std::runtime_error("rows has to be >= 1");
        if (C < 8 || (C & 7)) throw std::runtime_error("C = " + std::to_string(C) + " is not a multiple of 8");
        if (ldv < C || ldo < C || (ldv & 7) || (ldo & 7) || ((uintptr_t)v & 15) || ((uintptr_t)o & 15))
            throw std::runtime_error("every row stride has to be a multiple of 8 and >= C, every pointer 16-byte aligned");
        const int rc = ladi_launch_pag_identity(reinterpret_cast<const h16*>(v), ldv, reinterpret_cast<h16*>(o), ldo, rows, C, S(stream));
        if (rc) throw std::runtime_error("launch refused or failed (rc = " + std::to_string(rc) + ")");
        return 0;
    });
}
static int sched_run_any(const char* name, int kind, int steps, const float* ac_host, const void* eps_seq, int evals, int B, int hw, int cfg,
                         float guidance, float* latents, const float* step_noise, int noise_steps, float eta, void* stream) {
    return guarded(name, [&]() {
        hipStream_t st = S(stream);
        std::vector<float> ac;
        if (ac_host) ac.assign(ac_host, ac_host + 1000); else default_alphas_cumprod(ac);
        std::vector<double> ts; std::vector<StepTable> tb;
        build_step_table(kind, steps, ac.data(), 1 << 30, ts, tb, nullptr, eta);
        if (evals > (int)tb.size()) throw std::runtime_error("evals exceeds scheduler length");
        if (table_needs_step_noise(tb) && (!step_noise || noise_steps < evals))
            throw std::runtime_error("EulerAncestralDiscrete / DDIM with eta > 0 / LCM / TCD with eta > 0 need step noise for every evaluation run");
        char* buf = nullptr;
        const size_t plane = (size_t)B * hw * 4 * sizeof(float);
        const size_t tb_bytes = (tb.size() * sizeof(StepTable) + 255) & ~(size_t)255;
        HIP_OK(hipMalloc(reinterpret_cast<void**>(&buf), tb_bytes + 256 + 5 * plane));
        StepTable* dt = reinterpret_cast<StepTable*>(buf);
        int* dstep = reinterpret_cast<int*>(buf + tb_bytes);
        float* cur = reinterpret_cast<float*>(buf + tb_bytes + 256);
        float* ets = cur + (size_t)B * hw * 4;
        HIP_OK(hipMemcpyAsync(dt, tb.data(), tb.size() * sizeof(StepTable), hipMemcpyHostToDevice, st));
        HIP_OK(hipMemsetAsync(dstep, 0, 8, st));       // evaluation index + the step kernel's arrival ticket
        const int rows = (cfg ? 2 : 1) * B * hw;
        int rc = 0;
        for (int i = 0; i < evals && !rc; ++i) {
            StepArgs sa; std::memset(&sa, 0, sizeof(sa));
            sa.eps = reinterpret_cast<const h16*>(eps_seq) + (size_t)i * rows * 4; sa.ld_eps = 4;
            sa.B = B; sa.hw = hw; sa.cfg = cfg; sa.guidance = guidance; sa.latents = latents; sa.cur_sample = cur; sa.ets = ets;
            sa.table = dt; sa.step_idx = dstep; sa.unet_in = nullptr; sa.step_noise = step_noise;
            rc = ladi_launch_sched_step(sa, st);
        }
        HIP_OK(hipStreamSynchronize(st));
        (void)hipFree(buf);
        return rc;
    });
}
int ladi_op_sched_run(int kind, int steps, const float* ac_host, const void* eps_seq, int evals, int B, int hw, int cfg, float guidance,
                      float* latents, void* stream) {
    return sched_run_any("ladi_op_sched_run", kind, steps, ac_host, eps_seq, evals, B, hw, cfg, guidance, latents, nullptr, 0, 0.f, stream);
}
int ladi_op_sched_run_noise(int kind, int steps, const float* ac_host, const void* eps_seq, int evals, int B, int hw, int cfg, float guidance,
                            float* latents, const float* step_noise, int noise_steps, void* stream) {
    return sched_run_any("ladi_op_sched_run_noise", kind, steps, ac_host, eps_seq, evals, B, hw, cfg, guidance, latents, step_noise, noise_steps,
                         0.f, stream);
}
int ladi_op_sched_run_noise_eta(int kind, int steps, const float* ac_host, float eta, const void* eps_seq, int evals, int B, int hw, int cfg,
                                float guidance, float* latents, const float* step_noise, int noise_steps, void* stream) {
    return sched_run_any("ladi_op_sched_run_noise_eta", kind, steps, ac_host, eps_seq, evals, B, hw, cfg, guidance, latents, step_noise,
                         noise_steps, eta, stream);
}
int ladi_op_cfg_stats(const void* eps, int ld_eps, int B, int hw, float guidance, float phi, float* factor, void* stream) {
    return guarded("ladi_op_cfg_stats", [&]() {
        if (!eps || !factor || B <= 0 || hw <= 0) throw std::runtime_error("null argument or empty shape");
        if (ld_eps < 4 || (ld_eps & 3) || ((uintptr_t)eps & 7)) throw std::runtime_error("ld_eps must be a multiple of 4 (>= 4) and eps 8-byte aligned");
        if (!(phi >= 0.f && phi <= 1.f)) throw std::runtime_error("phi outside [0, 1]");
        return ladi_launch_cfg_stats(reinterpret_cast<const h16*>(eps), ld_eps, B, hw, nullptr, nullptr, guidance, phi, factor, S(stream));
    });
}
// cfg / pag_tab_host: ladi_op_sched_run_pag's (the others: cfg = 1, no PAG table).  Without CFG the guidance table may be null
static int sched_run_guided_any(const char* name, int kind, int steps, const float* ac_host, float eta, const void* eps_seq, int ld_eps, int evals,
                                int B, int hw, const float* guidance_tab_host, float phi, float* latents, const float* step_noise, int noise_steps,
                                const float* keep_x0, const float* keep_noise, const float* keep_mask, void* stream, int cfg = 1,
                                const float* pag_tab_host = nullptr, const float* sag_scale_host = nullptr) {
    return guarded(name, [&]() {
        hipStream_t st = S(stream);
        if (sag_scale_host && pag_tab_host) throw std::runtime_error("a PAG table together with a SAG scale");
        if (sag_scale_host && (!std::isfinite(*sag_scale_host) || *sag_scale_host < 0.f)) throw std::runtime_error("SAG scale negative or not finite");
        std::vector<float> ones;
        if (!cfg && !guidance_tab_host && evals > 0) { ones.assign((size_t)evals, 1.f); guidance_tab_host = ones.data(); }
        if (!eps_seq || !latents || !guidance_tab_host || evals <= 0 || B <= 0 || hw <= 0) throw std::runtime_error("null argument or empty shape");
        for (int i = 0; pag_tab_host && i < evals; ++i)
            if (!std::isfinite(pag_tab_host[i]) || pag_tab_host[i] < 0.f) throw std::runtime_error("PAG table entry negative or not finite");
        if (ld_eps < 4 || (ld_eps & 3) || ((uintptr_t)eps_seq & 7)) throw std::runtime_error("ld_eps must be a multiple of 4 (>= 4) and eps_seq 8-byte aligned");
        if (!(phi >= 0.f && phi <= 1.f)) throw std::runtime_error("phi outside [0, 1]");
        for (int i = 0; i < evals; ++i)
            if (!std::isfinite(guidance_tab_host[i]) || guidance_tab_host[i] < 0.f) throw std::runtime_error("guidance table entry negative or not finite");
        std::vector<float> ac;
        if (ac_host) ac.assign(ac_host, ac_host + 1000); else default_alphas_cumprod(ac);
        std::vector<double> ts; std::vector<StepTable> tb;
        build_step_table(kind, steps, ac.data(), 1 << 30, ts, tb, nullptr, eta);
        if (evals > (int)tb.size()) throw std::runtime_error("evals exceeds scheduler length");
        if (table_needs_step_noise(tb) && (!step_noise || noise_steps < evals))
            throw std::runtime_error("EulerAncestralDiscrete / DDIM with eta > 0 / LCM / TCD with eta > 0 need step noise for every evaluation run");
        char* buf = nullptr;
        const size_t plane = (size_t)B * hw * 4 * sizeof(float);
        const size_t tb_bytes = (tb.size() * sizeof(StepTable) + 255) & ~(size_t)255;
        const size_t gt_bytes = ((size_t)evals * sizeof(float) + 255) & ~(size_t)255;
        const size_t fc_bytes = ((size_t)B * sizeof(float) + 255) & ~(size_t)255;
        // the latent blend's coefficients, one row per evaluation of the whole run (evals may stop earlier)
        std::vector<float> kt;
        if (keep_mask) build_keep_coeffs(kind, steps, ac.data(), 0, kt);
        const size_t kt_bytes = (kt.size() * sizeof(float) + 255) & ~(size_t)255;
        const size_t pt_bytes = pag_tab_host ? gt_bytes : sag_scale_host ? 256 : 0;
        HIP_OK(hipMalloc(reinterpret_cast<void**>(&buf), tb_bytes + 256 + gt_bytes + fc_bytes + kt_bytes + 5 * plane + pt_bytes));
        StepTable* dt = reinterpret_cast<StepTable*>(buf);
        int* dstep = reinterpret_cast<int*>(buf + tb_bytes);
        float* dgt = reinterpret_cast<float*>(buf + tb_bytes + 256);
        float* dfc = reinterpret_cast<float*>(buf + tb_bytes + 256 + gt_bytes);
        float* dkt = reinterpret_cast<float*>(buf + tb_bytes + 256 + gt_bytes + fc_bytes);
        float* cur = reinterpret_cast<float*>(buf + tb_bytes + 256 + gt_bytes + fc_bytes + kt_bytes);
        float* ets = cur + (size_t)B * hw * 4;
        float* dpt = pag_tab_host ? ets + (size_t)4 * B * hw * 4 : nullptr;
        float* dsg = sag_scale_host ? ets + (size_t)4 * B * hw * 4 : nullptr;     // the SAG scale's device word, where a PAG table would stand
        int rc = 0;
        try {
            if (dpt) HIP_OK(hipMemcpyAsync(dpt, pag_tab_host, (size_t)evals * sizeof(float), hipMemcpyHostToDevice, st));
            if (dsg) HIP_OK(hipMemcpyAsync(dsg, sag_scale_host, sizeof(float), hipMemcpyHostToDevice, st));
            if (keep_mask) HIP_OK(hipMemcpyAsync(dkt, kt.data(), kt.size() * sizeof(float), hipMemcpyHostToDevice, st));
            HIP_OK(hipMemcpyAsync(dt, tb.data(), tb.size() * sizeof(StepTable), hipMemcpyHostToDevice, st));
            HIP_OK(hipMemcpyAsync(dgt, guidance_tab_host, (size_t)evals * sizeof(float), hipMemcpyHostToDevice, st));
            HIP_OK(hipMemsetAsync(dstep, 0, 8, st));       // evaluation index + the step kernel's arrival ticket
            const size_t per_eval = (size_t)((cfg ? 2 : 1) + (dpt || dsg ? 1 : 0)) * B * hw * ld_eps;
            for (int i = 0; i < evals && !rc; ++i) {
                StepArgs sa; std::memset(&sa, 0, sizeof(sa));
                sa.eps = reinterpret_cast<const h16*>(eps_seq) + (size_t)i * per_eval; sa.ld_eps = ld_eps;
                sa.B = B; sa.hw = hw; sa.cfg = cfg ? 1 : 0; sa.latents = latents; sa.cur_sample = cur; sa.ets = ets;
                sa.table = dt; sa.step_idx = dstep; sa.unet_in = nullptr; sa.step_noise = step_noise;
                sa.guidance_tab = dgt; sa.factor = (cfg && phi > 0.f) ? dfc : nullptr; sa.pag_tab = dpt; sa.sag_scale = dsg;
                if (keep_mask) { sa.keep_x0 = keep_x0; sa.keep_noise = keep_noise; sa.keep_mask = keep_mask; sa.keep_tab = dkt; }
                if (cfg && phi > 0.f && guidance_tab_host[i] > 1.0f)
                    rc = dsg ? ladi_launch_cfg_stats_sag(sa.eps, ld_eps, B, hw, dgt, dstep, 0.f, dsg, 0.f, phi, dfc, st)
                       : dpt ? ladi_launch_cfg_stats_pag(sa.eps, ld_eps, B, hw, dgt, dstep, 0.f, dpt, 0.f, phi, dfc, st)
                             : ladi_launch_cfg_stats(sa.eps, ld_eps, B, hw, dgt, dstep, 0.f, phi, dfc, st);
                if (!rc) rc = ladi_launch_sched_step(sa, st);
            }
            HIP_OK(hipStreamSynchronize(st));
        } catch (...) { (void)hipFree(buf); throw; }
        (void)hipFree(buf);
        return rc;
    });
}
int ladi_op_sched_run_guided(int kind, int steps, const float* ac_host, float eta, const void* eps_seq, int ld_eps, int evals, int B, int hw,
                             const float* guidance_tab_host, float phi, float* latents, const float* step_noise, int noise_steps, void* stream) {
    return sched_run_guided_any("ladi_op_sched_run_guided", kind, steps, ac_host, eta, eps_seq, ld_eps, evals, B, hw, guidance_tab_host, phi, latents,
                                step_noise, noise_steps, nullptr, nullptr, nullptr, stream);
}
int ladi_op_sched_run_pag(int kind, int steps, const float* ac_host, float eta, const void* eps_seq, int ld_eps, int evals, int B, int hw, int cfg,
                          const float* guidance_tab_host, const float* pag_tab_host, float phi, float* latents, const float* step_noise,
                          int noise_steps, void* stream) {
    if (!pag_tab_host) { set_error("ladi_op_sched_run_pag: null PAG table"); return -1; }
    return sched_run_guided_any("ladi_op_sched_run_pag", kind, steps, ac_host, eta, eps_seq, ld_eps, evals, B, hw, guidance_tab_host, phi, latents,
                                step_noise, noise_steps, nullptr, nullptr, nullptr, stream, cfg ? 1 : 0, pag_tab_host);
}
int ladi_op_cfg_stats_pag(const void* eps, int ld_eps, int B, int hw, float guidance, float pag_scale, float phi, float* factor, void* stream) {
    return guarded("ladi_op_cfg_stats_pag", [&]() {
        if (!eps || !factor || B <= 0 || hw <= 0) throw std::runtime_error("null argument or empty shape");
        if (ld_eps < 4 || (ld_eps & 3) || ((uintptr_t)eps & 7)) throw std::runtime_error("ld_eps must be a multiple of 4 (>= 4) and eps 8-byte aligned");
        if (!(phi >= 0.f && phi <= 1.f)) throw std::runtime_error("phi outside [0, 1]");
        if (!std::isfinite(pag_scale) || pag_scale < 0.f) throw std::runtime_error("PAG scale negative or not finite");
        return ladi_launch_cfg_stats_pag(reinterpret_cast<const h16*>(eps), ld_eps, B, hw, nullptr, nullptr, guidance, nullptr, pag_scale, phi, factor,
                                         S(stream));
    });
}
int ladi_op_sched_run_sag(int kind, int steps, const float* ac_host, float eta, const void* eps_seq, int ld_eps, int evals, int B, int hw, int cfg,
                          const float* guidance_tab_host, float sag_scale, float phi, float* latents, const float* step_noise, int noise_steps,
                          void* stream) {
    return sched_run_guided_any("ladi_op_sched_run_sag", kind, steps, ac_host, eta, eps_seq, ld_eps, evals, B, hw, guidance_tab_host, phi, latents,
                                step_noise, noise_steps, nullptr, nullptr, nullptr, stream, cfg ? 1 : 0, nullptr, &sag_scale);
}
int ladi_op_cfg_stats_sag(const void* eps, int ld_eps, int B, int hw, float guidance, float sag_scale, float phi, float* factor, void* stream) {
    return guarded("ladi_op_cfg_stats_sag", [&]() {
        if (!eps || !factor || B <= 0 || hw <= 0) throw std::runtime_error("null argument or empty shape");
        if (ld_eps < 4 || (ld_eps & 3) || ((uintptr_t)eps & 7)) throw std::runtime_error("ld_eps must be a multiple of 4 (>= 4) and eps 8-byte aligned");
        if (!(phi >= 0.f && phi <= 1.f)) throw std::runtime_error("phi outside [0, 1]");
        if (!std::isfinite(sag_scale) || sag_scale < 0.f) throw std::runtime_error("SAG scale negative or not finite");
        return ladi_launch_cfg_stats_sag(reinterpret_cast<const h16*>(eps), ld_eps, B, hw, nullptr, nullptr, guidance, nullptr, sag_scale, phi, factor,
                                         S(stream));
    });
}
int ladi_op_sag_map(const void* q, int ldq, long long sq, const void* k, int ldk, long long sk, int n, int T, int heads, float* s_out,
                    unsigned char* m_out, void* stream) {
    return guarded("ladi_op_sag_map", [&]() {
        if (!q || !k || !s_out || !m_out) throw std::runtime_error("null argument");
        if (n < 1 || T < 1 || heads < 1) throw std::runtime_error("n, T and heads have to be >= 1");
        if (ldq < heads * 64 || ldk < heads * 64 || (ldq & 7) || (ldk & 7) || (sq & 7) || (sk & 7) || ((uintptr_t)q & 15) || ((uintptr_t)k & 15))
            throw std::runtime_error("every stride has to be a multiple of 8, the row strides >= 64 * heads, both bases 16-byte aligned");
        hipStream_t st = S(stream);
        float* part = nullptr;
        HIP_OK(hipMalloc(reinterpret_cast<void**>(&part), (size_t)ladi_sag_partial_floats(n, T, heads) * sizeof(float)));
        const int rc = ladi_launch_sag_map(reinterpret_cast<const h16*>(q), ldq, sq, reinterpret_cast<const h16*>(k), ldk, sk, n, T, heads, part, s_out,
                                           m_out, st);
        const hipError_t e = hipStreamSynchronize(st);
        (void)hipFree(part);
        if (rc) throw std::runtime_error("launch refused or failed (rc = " + std::to_string(rc) + ")");
        HIP_OK(e);
        return 0;
    });
}
int ladi_op_sag_degrade(const float* latents, const void* eps, int ld_eps, const unsigned char* mask, int B, int h, int w, int hm, int wm,
                        float sqrt_a, float sqrt_1ma, float in_scale, const void* src_rows, void* dst_rows, int ld_in, int copy_end, void* stream) {
    return guarded("ladi_op_sag_degrade", [&]() {
        if (!latents || !eps || !mask || !dst_rows) throw std::runtime_error("null argument");
        if (B < 1 || hm < 1 || wm < 1) throw std::runtime_error("B, hm and wm have to be >= 1");
        if (h < 5 || w < 5) throw std::runtime_error("latents of " + std::to_string(h) + " x " + std::to_string(w) + " are under 5 x 5 (the blur's reflect padding)");
        if (!(sqrt_a > 0.f) || !std::isfinite(sqrt_a) || !std::isfinite(sqrt_1ma) || !std::isfinite(in_scale)) throw std::runtime_error("sqrt(a) has to be positive and every coefficient finite");
        hipStream_t st = S(stream);
        float* tab = nullptr;
        HIP_OK(hipMalloc(reinterpret_cast<void**>(&tab), 256));
        const float row[4] = {sqrt_a, sqrt_1ma, in_scale, 0.f};
        int rc = hipMemcpyAsync(tab, row, sizeof(row), hipMemcpyHostToDevice, st) == hipSuccess ? 0 : -100;
        if (!rc) rc = ladi_launch_sag_degrade(latents, reinterpret_cast<const h16*>(eps), ld_eps, mask, B, h, w, hm, wm, tab, nullptr,
                                              reinterpret_cast<const h16*>(src_rows), reinterpret_cast<h16*>(dst_rows), ld_in, copy_end, st);
        const hipError_t e = hipStreamSynchronize(st);
        (void)hipFree(tab);
        if (rc) throw std::runtime_error("launch refused or failed (rc = " + std::to_string(rc) + ")");
        HIP_OK(e);
        return 0;
    });
}
int ladi_op_sched_run_keep(int kind, int steps, const float* ac_host, float eta, const void* eps_seq, int ld_eps, int evals, int B, int hw,
                           const float* guidance_tab_host, float phi, float* latents, const float* step_noise, int noise_steps,
                           const float* keep_x0, const float* keep_noise, const float* keep_mask, void* stream) {
    if (!keep_x0 || !keep_noise || !keep_mask) { set_error("ladi_op_sched_run_keep: null keep_x0, keep_noise or keep_mask"); return -1; }
    if (((uintptr_t)keep_x0 | (uintptr_t)keep_noise) & 15) { set_error("ladi_op_sched_run_keep: keep_x0 and keep_noise must be 16-byte aligned"); return -1; }
    return sched_run_guided_any("ladi_op_sched_run_keep", kind, steps, ac_host, eta, eps_seq, ld_eps, evals, B, hw, guidance_tab_host, phi, latents,
                                step_noise, noise_steps, keep_x0, keep_noise, keep_mask, stream);
}
int ladi_op_mask_pool8(const void* mask_bin, int B, int H, int W, int invert, float* out, void* stream) {
    return guarded("ladi_op_mask_pool8", [&]() {
        if (!mask_bin || !out) throw std::runtime_error("null mask or out");
        if (B < 1 || H < 8 || W < 8 || (H & 7) || (W & 7)) throw std::runtime_error("B >= 1, H and W multiples of 8");
        if ((uintptr_t)mask_bin & 15) throw std::runtime_error("the mask must be 16-byte aligned");
        if (ladi_launch_mask_pool8(reinterpret_cast<const h16*>(mask_bin), B, H, W, invert ? 1 : 0, out, S(stream))) throw std::runtime_error("launch refused or failed");
        return 0;
    });
}
int ladi_op_mask_feather(const void* mask_bin, int B, int H, int W, float sigma, float* tmp, float* out, void* stream) {
    return guarded("ladi_op_mask_feather", [&]() {
        if (!mask_bin || !tmp || !out || tmp == out) throw std::runtime_error("null mask, tmp or out (tmp and out must differ)");
        if (B < 1 || H < 1 || W < 1) throw std::runtime_error("every size has to be >= 1");
        if (!(sigma > 0.f) || !(sigma <= 32.f)) throw std::runtime_error("sigma " + std::to_string(sigma) + " outside (0, 32]");
        if (ladi_launch_mask_feather(reinterpret_cast<const h16*>(mask_bin), B, H, W, sigma, tmp, out, S(stream))) throw std::runtime_error("launch refused or failed");
        return ladi_feather_radius(sigma);
    });
}
int ladi_op_image_composite(const void* decoded, int ld, const void* image, int dtype, const void* mask, int mask_f32, int B, int HW, void* dst,
                            int dst_u8, void* stream) {
    return guarded("ladi_op_image_composite", [&]() {
        if (!decoded || !image || !mask || !dst) throw std::runtime_error("null argument");
        if (dtype != LADI_F32 && dtype != LADI_F16) throw std::runtime_error("image dtype must be fp32 or fp16");
        if (B < 1 || HW < 4 || (HW & 3)) throw std::runtime_error("B >= 1 and H * W a multiple of 4");
        if (ld < 4 || (ld & 3) || ((uintptr_t)decoded & 7)) throw std::runtime_error("ld must be a multiple of 4 (>= 4) and decoded 8-byte aligned");
        if (ladi_launch_image_composite(reinterpret_cast<const h16*>(decoded), ld, image, dtype == LADI_F32, mask, mask_f32 ? 1 : 0, B, HW, dst, dst_u8 ? 1 : 0,
                                        S(stream))) throw std::runtime_error("launch refused or failed");
        return 0;
    });
}

}  // extern "C"
