// libladi_native runtime: weight store, device pools, activation arena, op wrappers and the module graphs
// (extended SD2-inpainting UNet, EMASC-aware VAE, EMASC, inversion adapter, try-on pipeline).
// Internal header; the public boundary is include/ladi_native.h.
#pragma once
#include "kernels.h"
#include <string>
#include <vector>
#include <functional>
#include <cstring>
#include <unordered_map>
#include <memory>
#include <stdexcept>

namespace ladi {

void set_error(const std::string& msg);
const char* last_error();

// ------------------------------------------------------------------------------------------------
struct HostTensor {
    std::vector<int64_t> shape;
    std::vector<float> data;
    size_t numel() const { size_t n = 1; for (auto s : shape) n *= (size_t)s; return n; }
};
struct WeightStore {
    std::unordered_map<std::string, HostTensor> m;
    bool has(const std::string& k) const { return m.find(k) != m.end(); }
    const HostTensor& get(const std::string& k) const;  // throws std::runtime_error when missing
};

// persistent device memory (weights, caches): chunked bump allocator, freed with the owner
struct DevPool {
    std::vector<void*> chunks;
    char* cur = nullptr;
    size_t left = 0;
    size_t total = 0;
    void* alloc(size_t bytes);
    h16* upload_h16(const std::vector<float>& v);  // fp32 host -> fp16 device
    float* upload_f32(const std::vector<float>& v);
    ~DevPool();
};

// transient activations: stack-discipline bump arena with a dry-run (planning) mode
struct Arena {
    char* base = nullptr;
    size_t cap = 0, off = 0, peak = 0;
    bool dry = false;
    void* alloc(size_t bytes);
    size_t mark() const { return off; }
    void release(size_t m) { off = m; }
    void reserve(size_t bytes);  // (re)allocate backing store; not capturable
    ~Arena();
};

struct Act {  // NHWC fp16 activation view
    h16* p = nullptr;
    int n = 0, h = 0, w = 0, c = 0, ld = 0;
    // per-channel partial statistics written by the producing igemm (rows of st_px pixels, [rows][c][2] floats); st_px = 0: none
    float* st_part = nullptr; int st_px = 0;
    size_t pixels() const { return (size_t)n * h * w; }
};

// Opt-in fp16 range probe (probe.hip): one device slot {bits of the largest finite |x|, number of inf / NaN elements} per NAMED activation
// of the modules it is attached to (UNet / VAE / EMASC ::probe).  A name gets its slot the first time a planning (dry) pass meets it, so
// slot order is call order; the real pass only looks names up and launches the kernel on the pass's stream -- no allocation, no
// synchronisation, capturable.  Slots accumulate (max / sum) until reset().  Names are the diffusers key prefix of the producing module.
struct ProbeSlot { unsigned absmax_bits; unsigned nonfinite; };
struct Probe {
    int cap = 0;
    // never reused within the process: what a captured graph that holds this probe's launches is keyed on (a later Probe can get the same
    // device addresses back from the allocator with another name <-> slot order or a smaller cap)
    unsigned long long id = 0;
    ProbeSlot* d_slots = nullptr;            // device [cap]
    ProbeSlot* h_slots = nullptr;            // pinned host mirror [cap] (read())
    // d_rank[0]: how many slots have gone non-finite since the last reset; d_rank[1 + i]: the rank in time (1-based) at which slot i first held
    // an inf / NaN, 0 = never.  Slot order is the order of one forward; inside the denoising loop a NaN of evaluation k comes back into the
    // earlier slots at evaluation k + 1, so "which layer overflowed first" needs the time order
    unsigned* d_rank = nullptr; unsigned* h_rank = nullptr;
    std::vector<std::string> names;          // slot i <-> names[i]
    std::vector<float> scale;                // factor by which slot i's tensor is stored relative to its true value (last call's)
    std::unordered_map<std::string, int> index;
    explicit Probe(int max_points);
    ~Probe();
    void release();                          // frees the device / pinned buffers (destructor, failed construction)
    Probe(const Probe&) = delete;
    Probe& operator=(const Probe&) = delete;
    int slot(const std::string& name, bool add);                       // index of `name` (registered when add), -1: unknown
    void reset(hipStream_t st);                                        // zero every slot, asynchronous on st
    void reset_prefix(const char* prefix, hipStream_t st);             // zero the slots whose name starts with prefix
    // true-scale absmax (stored absmax / scale) and counts of the first min(count, cap_out) slots; synchronises st
    void read(float* absmax_out, unsigned* nonfinite_out, int cap_out, hipStream_t st);
    void read_rank(unsigned* rank_out, int cap_out, hipStream_t st);   // d_rank[1 + i] of the first min(count, cap_out) slots; synchronises st
};

struct Ctx {
    hipStream_t st = nullptr;
    Arena* ar = nullptr;
    float* stats = nullptr;  // GroupNorm statistics arena (floats), zeroed at forward start
    size_t stats_off = 0, stats_cap = 0, stats_peak = 0;
    int* bad = nullptr;      // optional device flag: set by a GroupNorm whose input statistics are not finite (fp16 overflow upstream)
    int* sk_cnt = nullptr;   // arrival counters of the in-launch split-K combine for THIS stream (1024 ints, zeroed once; kernels.h); null: process-wide
    bool dry() const { return ar->dry; }
    h16* alloc_h16(size_t elems) { return reinterpret_cast<h16*>(ar->alloc(elems * sizeof(h16))); }
    float* alloc_f32(size_t elems) { return reinterpret_cast<float*>(ar->alloc(elems * sizeof(float))); }
    float* alloc_stats(size_t floats);
    Act new_act(int n, int h, int w, int c, int ld = 0);
    void check(int rc, const char* what);
    // range probe of the module being run (set from the module's `probe` for the span of its forward; null = off: probe_point returns at
    // once and nothing is launched).  scale: the factor by which `a` is stored relative to its true value
    Probe* probe = nullptr;
    void probe_point(const char* name, const Act& a, float scale = 1.f);
};
// sets Ctx::probe for the span of one module's forward and puts the caller's back
struct ProbeScope {
    Ctx& c; Probe* saved;
    ProbeScope(Ctx& c_, Probe* p) : c(c_), saved(c_.probe) { c.probe = p; }
    ~ProbeScope() { c.probe = saved; }
};

// Two-pass (plan, run) execution of a module graph on its arena: `body(Ctx&)` runs once dry (addresses are fake, nothing is launched; it
// only records the arena / statistics peaks), the plan is committed, and it runs again for real.  Both passes must allocate identically.
// A body reports failure by throwing std::runtime_error (Ctx::check does).
// commit_plan: reserve the arena (peak + 4096 bytes) and grow the GroupNorm-statistics buffer to `stats_peak` floats (stats may be null)
void commit_plan(Arena& arena, size_t stats_peak, float** stats, size_t* stats_cap);
// stats / stats_cap: the owner's statistics buffer (grown here, zeroed at the start of the real pass) or null; sk_cnt: see Ctx::sk_cnt
template <typename Body>
void run_planned(Arena& arena, hipStream_t st, Body&& body, float** stats = nullptr, size_t* stats_cap = nullptr, int* sk_cnt = nullptr) {
    for (int pass = 0; pass < 2; ++pass) {
        arena.dry = (pass == 0);
        arena.off = 0;
        Ctx c; c.st = st; c.ar = &arena; c.sk_cnt = sk_cnt;
        if (stats) { c.stats = *stats; c.stats_cap = *stats_cap; }
        if (pass == 1 && c.stats_cap && hipMemsetAsync(c.stats, 0, c.stats_cap * sizeof(float), st) != hipSuccess)
            throw std::runtime_error("run_planned: zeroing the GroupNorm statistics failed");
        body(c);
        if (pass == 0) commit_plan(arena, c.stats_peak, stats, stats_cap);
    }
}

// ------------------------------------------------------------------------------------------------
struct DConv {  // conv3x3 / conv1x1 / linear weights in igemm layout [cout][k*k][cin_pad]
    h16* w = nullptr; h16* b = nullptr;
    int cin = 0, cin_pad = 0, cout = 0, k = 1;
    int K() const { return k * k * cin_pad; }
};
struct DNorm { h16* g = nullptr; h16* b = nullptr; int c = 0; };

struct ConvOpt {
    int stride = 1, pad = -1 /* -1: k/2 */, ups = 0, act = LADI_ACT_NONE;
    int pad_end = -1;        // trailing (bottom / right) pad of a strided conv, -1: = pad (the VAE's F.pad(0, 1, 0, 1) downsamplers: 1 with pad 0)
    int ups_h = 0, ups_w = 0;   // ups: size the source is stretched to (nearest, diffusers' `upsample_size`); 0: twice the source
    const float* rowadd = nullptr; const int* rowadd_idx = nullptr; int rowadd_stride = 0;
    const Act* res0 = nullptr; const Act* res1 = nullptr;
    const h16* mask = nullptr;
    float out_scale = 1.f;
    float bias_mul = 0.f;    // multiplier of the bias (0 = 1), see IGemmArgs::bias_mul
    int out_ld = 0;          // 0 -> cout (GEGLU: cout/2)
    int cfg = 0;             // igemm tile config override
    bool stats = false;      // also produce per-channel partial statistics of the output (for a consuming GroupNorm)
    Act* dst = nullptr;      // caller-owned output view of the computed size: nothing is allocated for the output (out_ld and stats are the
                             // view's: ld, st_part); its st_part / st_px are updated like the returned Act's
    const DNorm* ln = nullptr; float ln_eps = 1e-5f;   // LayerNorm applied to the input first: fused into the kernel when it can be, else a launch
    const float* gn_ss = nullptr;                      // GroupNorm affine of the input ([n][C][2] scale / shift from gn_scale_shift) applied
                                                       // in the X-stationary kernel's prologue (see gn_fusable)
};

DConv load_conv(DevPool& pool, const WeightStore& ws, const std::string& prefix, int cin_expected = -1);      // 4-D or 2-D weight
DConv load_linear_cat(DevPool& pool, const WeightStore& ws, const std::vector<std::string>& prefixes, bool bias);  // row-concat
DConv load_geglu(DevPool& pool, const WeightStore& ws, const std::string& prefix);
DNorm load_norm(DevPool& pool, const WeightStore& ws, const std::string& prefix);

Act conv2d(Ctx& c, const DConv& cv, const Act& x, const Act* x2, const ConvOpt& o);
// output tensor + worst-case partial-statistics buffer (rows of 32 pixels) allocated together (stack discipline)
Act new_act_with_stats(Ctx& c, int n, int h, int w, int cc);
// dst: caller-owned dense output view [n, h, w, C0 + C1] (null: allocated from the arena)
Act group_norm(Ctx& c, const DNorm& nm, const Act& x, const Act* x2, int groups, float eps, int silu, const Act* add = nullptr,
               const Act* dst = nullptr);
// statistics + finalize only: per-(sample, channel) scale / shift of GroupNorm(x | x2) as [n][C0 + C1][2] floats (what group_norm applies)
float* gn_scale_shift(Ctx& c, const DNorm& nm, const Act& x, const Act* x2, int groups, float eps);
// can a following 1x1 projection apply that affine in its own prologue instead of a gn_apply pass?  (X-stationary kernel: K = 320 / 640,
// whole 128-pixel panels, 32-pixel blocks inside one sample); LADI_GN_FUSE=0 switches it off (A/B)
bool gn_fusable(const Act& x, int cout);
Act layer_norm(Ctx& c, const DNorm& nm, const Act& x, float eps);

// ------------------------------------------------------------------------------------------------
struct ResBlock {
    DNorm n1, n2; DConv c1, c2, sc; bool has_sc = false; int cin = 0, cout = 0; int temb_off = -1;
};
struct XfBlock {
    DNorm gn, ln1, ln2, ln3; DConv proj_in, qkv, o1, q2, kv2, o2, ff1, ff2, proj_out; int C = 0, heads = 0;
    // the block's place in the UNet (UNet::xf, filled by UNet::load): its index in execution order -- the bit of UNet::pag_mask, the slot of
    // ToMe::out_row, the position of its IP-Adapter scale --, its resolution level 0 .. 3 and its diffusers prefix (down_blocks.0.attentions.1)
    int bit = 0, level = 0; std::string prefix;
    h16* kv_cache = nullptr;  // [n][L][2C]
    // fused sub-blocks of the C = 320 level (xf_fused.hip): operands packed once at load (o2_packed, ff2_packed) / per context (kp, vt)
    h16* o2_packed = nullptr; h16* ff2_packed = nullptr; h16* kp_tiles = nullptr; h16* vt_tiles = nullptr;
    // IP-Adapter (UNet::ip_load): attn2.processor.to_k_ip | to_v_ip packed like kv2, the image K/V of the image context [n][N][2C], and this
    // block's scale (0: the block launches nothing for the image term)
    DConv ip_kv; h16* ip_kv_cache = nullptr; float ip_scale = 1.f;
};

struct UNetCfg {
    int in_channels = 31, out_channels = 4;
    int boc[4] = {320, 640, 1280, 1280};
    int heads[4] = {5, 10, 20, 20};
    int layers_per_block = 2;
    int cross_dim = 1024;
    int groups = 32;
    float eps = 1e-5f;
};

// Deep-feature cache of the 64x48 level (DeepCache, level 0 only).  A whole forward in mode CAPTURE copies the hidden state that enters
// up_blocks.3.resnets.(L - branch) -- before the concatenation with its skip -- into `buf`; a forward in mode SHALLOW runs conv_in, layers
// 0 .. branch-1 of down_blocks.0, then up_blocks.3 layers L-branch .. L from that tensor, conv_norm_out and conv_out, and nothing else.
// That tensor has boc[0] channels for branch < L (an output of up_blocks.3) and boc[1] for branch = L (the output of up_blocks.2's
// upsampler): UNet::fc_channels.
// buf: caller-owned fp16 [samples of the context batch][h][w][fc_channels(branch)]; a forward reads / writes the rows of its own samples
// (sample0, as the cross-attention K/V cache), so sub-batch forwards (cond-only evaluations, sample-group lanes) share one buffer.  The
// cached half brings no statistics rows: the consuming GroupNorm recomputes them (gn_partial), as for any source without producer rows.
struct FeatCache {
    enum { NONE = 0, CAPTURE = 1, SHALLOW = 2 };
    int mode = NONE, branch = 0;
    h16* buf = nullptr;
};

// FreeU (diffusers enable_freeu; ladi_unet_set_freeu, sticky, off by default).  Before every concatenation cat([hidden, skip]) of
// up_blocks.0 (b1, s1) and up_blocks.1 (b2, s2) -- 2 x (layers_per_block + 1) sites -- the first half of the hidden state's channels is
// multiplied by b and the skip's lowest frequencies by s, one launch per site (freeu.hip), in place: both tensors have this resnet as
// their only remaining reader.  Off launches exactly the plain forward.  A captured graph of the forward is keyed on all five fields
struct FreeU {
    bool on = false;
    float s1 = 1.f, s2 = 1.f, b1 = 1.f, b2 = 1.f;
};

// Perturbed-attention guidance (diffusers PAGMixin): the context index from which a forward's samples are perturbed.  In the transformer
// blocks selected by UNet::pag_mask a perturbed sample's self-attention map is the identity (pag.hip); everything else is untouched
enum { PAG_NONE = 0x7fffffff };

// The optional arguments of UNet::forward and UNetLanes::forward (which sets eps_out per lane itself)
// eps_out: pre-allocated output view (rows of a shared buffer); sample0: index of x's first sample in the context batch
// fc: deep-feature cache mode of this forward (FeatCache); null or mode NONE launches exactly the plain forward
// pag_first: samples whose index in the context batch (the numbering of sample0) is >= pag_first are perturbed; a forward's own count of
// leading unperturbed samples is clamp(pag_first - sample0, 0, n), every lane clamps it to its own samples.  Arena use does not depend on it
// sag: capture the SAG map in this forward (UNet::sag_capture): -1 = the UNet's sticky flag, 0 = no, 1 = yes
struct FwdOpt {
    const Act* eps_out = nullptr; int sample0 = 0; const FeatCache* fc = nullptr; int pag_first = PAG_NONE; int sag = -1;
};

// Token merging (tomesd.apply_patch; ladi_unet_set_token_merging, sticky, off by default; tome.hip, DESIGN.md "Token merging").  In the
// transformer blocks of the first max_downsample levels the selected sub-layers run over T - r rows: one plan per block and forward, from
// the block's token input (the output of proj_in), reused by all its merged sub-layers.  Level state (the dst / src tables, one persistent
// out_row buffer per block of the level) is built by a planning pass when the configuration, the level's size or the sample capacity is
// first seen -- never by a real pass, so never inside a capture -- and `gen` counts the rebuilds: a captured graph is keyed on the
// configuration and on gen.  r = 0 (ratio 0, or a level of a single row or column): the block runs the plain path launch for launch
struct ToMeCfg {
    double ratio = 0.0;
    int max_downsample = 1, sx = 2, sy = 2, use_rand = 0;
    unsigned seed = 0;
    int merge_attn = 1, merge_crossattn = 0, merge_mlp = 0;
};
struct ToMeLevel {
    int h = 0, w = 0, T = 0, Ns = 0, Nd = 0, r = 0, cap_n = 0;
    int* src_pos = nullptr; int* dst_pos = nullptr;       // device tables
    void* mem = nullptr;                                  // one allocation: the tables and the level's out_row buffers (freed by the UNet)
};
struct ToMe {
    bool on = false;
    ToMeCfg cfg;
    ToMeLevel lv[2];
    int* out_row[32] = {};                                // per transformer block (PAG's bit numbering): [cap_n][T] of its level
    unsigned long long gen = 0;
};
// the refusal of a configuration, or an empty string (ratio 0 is valid: off)
std::string tome_cfg_error(const ToMeCfg& c);

// LoRA (runtime_lora.cpp; DESIGN.md "LoRA").  A target is one diffusers conv / linear module: a block of rows of one packed weight.  The
// concatenated weights (qkv, kv2, temb_all) hold one target per member module, the GEGLU projection is one target with the interleaved
// row map.  Adapters keep their factors on the device in fp32; set_adapters re-merges every touched block from the pristine copy of its
// packed weight (taken the first time an adapter touches it), so weights never move and nothing drifts.
struct LoraTarget {
    std::string name;                       // diffusers module name, e.g. down_blocks.0.attentions.0.transformer_blocks.0.attn1.to_q
    DConv* cv = nullptr;                    // the packed weight the block lives in
    int row0 = 0, rows = 0, geglu_half = 0; // block of rows (kernels.h LoraMergeArgs)
    XfBlock* xf = nullptr; int packed = 0;  // 1 / 2: the block's attn2.to_out.0 / ff.net.2, which the fused sub-blocks read re-packed
};
struct LoraFactor { int rank = 0; float alpha = 0.f; const float* up = nullptr; const float* down = nullptr; };
struct LoraAdapter {
    std::string name;
    float* dev = nullptr;                   // one allocation: every factor of the adapter
    std::unordered_map<int, LoraFactor> f;  // target index -> factors
    ~LoraAdapter();
};

// IP-Adapter Plus image projection: the tencent-ailab `Resampler` (Perceiver resampler), restated from memory of that package, not checked
// against it (runtime_resampler.cpp has the arithmetic).  Geometry comes from the weights: N latents of width dim, input width E, `depth`
// layers of heads = inner / dim_head attention heads over T + N keys and a bias-free 4x GELU feed-forward, output width out_dim
struct ResamplerLayer { DNorm n1, n2, ffn; DConv q, kv, o, w1, w2; };
struct Resampler {
    DevPool pool;
    int N = 0, E = 0, dim = 0, depth = 0, heads = 0, dim_head = 0, out_dim = 0;
    h16* latents = nullptr;                  // [N][dim]
    DConv proj_in, proj_out; DNorm norm_out; std::vector<ResamplerLayer> layers;
    Arena arena;
    // prefix: what stands before the original keys ("" or "image_proj.").  check: host only -- every key, shape and limit
    // (include/ladi_native.h), throws with a message, else fills the geometry; upload: the weights of a checked store to the device
    void check(const WeightStore& ws, const std::string& prefix, int dim_head);
    void upload(const WeightStore& ws, const std::string& prefix);
    // x fp16 [n][T][E] dense -> tokens_out fp16 [n][N][out_dim] dense.  Throws on a launch failure
    void forward(const h16* x, int n, int T, h16* tokens_out, hipStream_t st);
};

struct UNet {
    UNetCfg cfg;
    std::vector<LoraTarget> lora_targets; std::unordered_map<std::string, int> lora_index;
    std::vector<std::unique_ptr<LoraAdapter>> lora_adapters;
    std::vector<std::pair<std::string, float>> lora_active;       // the active set, in merge order
    std::unordered_map<const h16*, h16*> lora_base;               // live packed weight -> its pristine copy (in `pool`)
    unsigned* lora_cnt = nullptr;                                 // device [lora_targets.size()]: non-finite results of the last merge, per target
    void build_lora_targets();                                    // end of load(): the vectors of blocks no longer move
    void lora_load(const std::string& name, const WeightStore& ws);
    void lora_delete(const std::string& name);
    // throws std::runtime_error (nothing changed, or -- non-finite results -- the previous set merged back)
    void lora_set(const std::vector<std::pair<std::string, float>>& set, hipStream_t st);
    long long export_weight(const std::string& key, float* host_out, long long cap);
    FreeU freeu;
    // IP-Adapter image prompt (diffusers load_ip_adapter / set_ip_adapter_scale / ip_adapter_image_embeds; DESIGN.md "IP-Adapter").  One adapter
    // per UNet: the image projection (Linear [N * cross_dim, E] + LayerNorm per token) and to_k_ip | to_v_ip of every transformer block, in
    // their own pool.  An image context (set_ip_context / set_ip_tokens) is the hoisted image K/V of every block for n samples of ip_ctx_N
    // tokens, in its own grow-only pool; with one set, attn2 of every block whose scale is not 0 adds scale * softmax(q k_ip^T / 8) v_ip to its
    // attention output before to_out (ip_adapter.hip), reading the rows of this forward's samples (sample0) as kv_cache is read.  Without an
    // image context the forward launches exactly the plain forward.  LoRA (lora_set) leaves all of it alone: no LoRA target is an image weight
    bool ip_loaded = false; int ip_N = 0, ip_E = 0;           // tokens per image and embedding width of the loaded projection
    std::unique_ptr<DevPool> ip_pool;
    h16* ip_proj_w = nullptr; h16* ip_proj_b = nullptr; DNorm ip_norm;
    int ip_ctx_n = 0, ip_ctx_N = 0; size_t ip_ctx_cap = 0;    // image context: samples (0 = none), tokens per sample; capacity in rows (n * N)
    std::unique_ptr<DevPool> ip_ctx_pool; h16* ip_lin = nullptr; h16* ip_tok = nullptr;   // projection output / tokens [rows][cross_dim]
    void ip_load(const WeightStore& ws, int dim_head = 64);   // throws; everything is checked before anything changes
    void ip_unload();
    void ip_set_scale(const float* scales, int count);        // throws on a wrong count or a non-finite value, nothing changed
    void ip_reserve(int n, int N);                            // host only: buffers for n samples of N tokens, and the context's shape (planning passes)
    int set_ip_context(const h16* embeds, int n, hipStream_t st);          // fp16 [n][ip_E] -> projection, LayerNorm, one igemm per block
    int set_ip_tokens(const h16* tokens, int n, int N, hipStream_t st);    // finished tokens fp16 [n][N][cross_dim]
    // Plus adapter: image_proj.* of the loaded weights is a Resampler (out_dim = cross_dim) instead of the Linear + LayerNorm; ip_N / ip_E are
    // its N and E.  set_ip_context is refused then, and set_ip_context_seq -- hidden states fp16 [n][T][ip_E] -> Resampler into ip_tok -> the
    // per-block K/V GEMMs -- is refused on a plain adapter.  ip_dim_head: the head width ip_load builds the Resampler with
    std::unique_ptr<Resampler> ip_resampler; int ip_dim_head = 64;
    int set_ip_context_seq(const h16* hidden, int n, int T, hipStream_t st);
    void clear_ip_context() { ip_ctx_n = 0; }
    // A/B switch of the image term (tools/bench_ip_adapter.py; ladi_unet_set_ip_route): 0 = ip_attn_add, the shipped route on every level
    // (BASELINE.md "IP-Adapter"); 1 = flash_attn64 over the N image keys into a scratch tensor plus ip_scaled_add (two roundings)
    int ip_route = 0;
    // pag_applied_layers (ladi_unet_set_pag_layers, sticky): bit i = transformer block i in execution order (xf[i].bit) -- down_blocks.{0,1,2}
    // .attentions.{0..L-1}, mid_block, up_blocks.{1,2,3}.attentions.{0..L}; pag_layer_count() bits.  The default is the mid block, as in
    // diffusers.  Without perturbed samples in a forward (pag_first = PAG_NONE) the mask has no effect
    unsigned pag_mask = 0;
    int pag_layer_count() const { return (int)xf.size(); }
    // token merging (ToMe above).  tome_blocks: the bits of the blocks the configuration merges, in execution order; tome_prepare: the
    // level state for a forward of samples [0, need_n) at h x w -- a planning pass builds it (synchronises the device and bumps gen when
    // something is freed), a real pass only checks it and throws
    ToMe tome;
    void tome_set(const ToMeCfg* c);                          // throws on a refused configuration, nothing changed; null / ratio 0: off
    std::vector<int> tome_blocks() const;
    const ToMeLevel* tome_prepare(int level, int h, int w, int need_n, bool dry);
    // self-attention guidance map (sag.hip; ladi_unet_set_sag_capture, sticky, off by default; DESIGN.md "Self-attention guidance").  A
    // capturing forward runs sag_map in mid_block.attentions.0's transformer block right after its attn1 Q / K projection and leaves
    // s fp32 [sample][T] and m bytes [sample][T] in sag_s / sag_m, at the rows of the forward's own samples in the context batch (sample0),
    // so lanes and sub-batch forwards share the buffers.  The buffers are grown by a planning pass only (sag_prepare, as tome_prepare) and
    // sag_gen counts the regrowths; with capture off nothing is allocated or launched.  sag_T: the token count of the last capture
    bool sag_capture = false;
    float* sag_s = nullptr; unsigned char* sag_m = nullptr; void* sag_mem = nullptr; int sag_T = 0, sag_cap_n = 0, sag_cap_T = 0;
    void sag_prepare(int T, int need_n, bool dry);
    // the mid block's map size for h x w latents: three stride-2 convolutions with padding 1, each ceil(x / 2)
    static void sag_tokens(int h, int w, int* hm, int* wm) {
        for (int i = 0; i < 3; ++i) { h = (h + 1) / 2; w = (w + 1) / 2; }
        *hm = h; *wm = w;
    }
    int mid_bit = 0;                                          // xf index of mid_block.attentions.0
    DevPool pool;
    DConv conv_in, conv_out, time_l1, time_l2, temb_all;
    DNorm norm_out;
    std::vector<ResBlock> down_res, up_res; ResBlock mid_res[2];
    // every transformer block in execution order: down 0 .. 2, mid, up 1 .. 3.  Filled by load() and never moved afterwards (LoraTarget
    // points into it); each block knows its own bit, level and prefix
    std::vector<XfBlock> xf;
    DConv down_samp[3], up_samp[3];
    int temb_total = 0;
    int xf_fuse = 0;                        // LADI_XF_FUSE, latched at load(): fused attn2 / feed-forward kernels of the C = 320 level (default off)
    // context (cross-attention K/V) cache
    int ctx_n = 0, ctx_L = 0, ctx_cap_n = 0, ctx_cap_samples = 0;    // cache capacity in rows (n * L) and, for the per-sample tiles, in samples
    std::unique_ptr<DevPool> ctx_pool;
    // time-embedding table
    float* temb_table = nullptr; int temb_rows_cap = 0; int temb_rows = 0;
    // own arena for the stand-alone forward entry
    Arena arena; float* stats = nullptr; size_t stats_cap = 0;
    h16* in_buf = nullptr; size_t in_cap = 0;
    Probe* probe = nullptr;                 // attached range probe (not owned): conv_in, every resnet / transformer / sampler output, conv_out

    void load(const UNetCfg& c, const WeightStore& ws);
    int set_context(const h16* ehs, int n, int L, hipStream_t st);
    int compute_temb(const float* timesteps_host, int count, hipStream_t st);  // fills temb_table rows [0,count)
    // x: [n,h,w,64] padded NHWC input; returns eps Act [n,h,w,4(ld 4)]
    Act forward(Ctx& c, const Act& x, const float* temb_row, const int* temb_idx, const FwdOpt& o = FwdOpt());
    // The UNet's part of the hipGraph key (GraphKey, whose rule it follows): every value a captured forward carries as an argument and one
    // representative pointer of every pool it dereferences (a pool's buffers are allocated together).  Plain data; key() fills a ZEROED Key,
    // and what belongs to a feature that is off stays zero.  perturbed: the run has perturbed samples -- only then does pag_mask reach a launch
    struct Key {
        const void *temb_table, *kv_cache;
        unsigned long long probe;                   // Probe::id (0 = none): a graph captured with a probe's launches is replayed only with that probe
        int freeu_on; unsigned freeu[4];            // s1, s2, b1, b2 by their bits
        unsigned pag_mask;
        int ip_on, ip_N; const void* ip_kv; unsigned ip_scale[32];     // tokens per sample, the image K/V, every block's scale by its bits
        int tome_on; int tome_opts[8]; unsigned long long tome_ratio, tome_gen;   // every configuration field and the generation of the level state
        int sag_on; const void* sag_buf;            // a forward of the graph captures the SAG map, into this buffer
    };
    // sag: -1 = the sticky flag decides (stand-alone forwards), else whether the owner's forwards capture the map (FwdOpt::sag)
    void key(Key& k, bool perturbed, int sag = -1) const;
    int fc_channels(int branch) const { return cfg.boc[branch >= cfg.layers_per_block ? 1 : 0]; }   // channels of the cached tensor
    // cache of the stand-alone entry ladi_unet_forward_cached: grow-only buffer over the context batch, the geometry it was captured at and
    // which sample rows hold a capture made since the last set_context
    h16* fc_buf = nullptr; size_t fc_cap = 0; int fc_h = 0, fc_w = 0, fc_branch = -1; std::vector<char> fc_rows;
    ~UNet();
};

// Sample-group lanes of one UNet forward.  No operation of the forward couples two samples (GroupNorm, LayerNorm and attention are
// per-sample; the CFG halves meet only in the scheduler kernel), so the n samples of a CFG-stacked batch are run as G independent
// forwards of n / G samples on G HIP streams, forked from and joined back into the caller's stream with events -- capturable: the
// denoising step becomes ONE hipGraph with G parallel branches.  Why: at batch 8 a single forward is a chain of ~410 dependent
// launches, many of which cannot fill 256 CUs (192 tiles of 320x256 on the 64x48 level, ~60-240 workgroups on the 8x6 level) and
// each of which pays its own ramp-up, drain and kernel boundary; two chains in flight fill each other's idle CUs and hide each
// other's boundaries.  Every lane owns its activation arena and GroupNorm-statistics buffer (planned by a dry run like every arena of
// this library), so lanes never share a transient address.
struct UNetLanes {
    static constexpr int MAXG = 8;
    int G = 1;
    hipStream_t st[MAXG] = {};              // st[0] unused: lane 0 runs on the caller's stream
    hipEvent_t fork = nullptr, join[MAXG] = {};
    Arena arena[MAXG]; size_t peak[MAXG] = {};
    float* stats[MAXG] = {}; size_t stats_cap[MAXG] = {}, stats_peak[MAXG] = {};
    int* sk_cnt[MAXG] = {};                 // per-lane split-K arrival counters (lanes run concurrently)
    static int pick(int n);                 // LADI_UNET_LANES (default 1), lowered until it divides n
    void configure(int n, int g = 0);       // g = 0: pick(n); creates the streams / events; a changed lane count drops the old plan
    void reset();                           // release every lane arena (streams / events / counters are kept)
    // x [n,h,w,64] -> eps [n,h,w,ld] (both caller-owned, contiguous in n).  dry: planning pass (records arena / statistics peaks, no
    // launches); concurrent = false runs the lanes one after the other on main_st (first evaluation: per-shape tile measurement wants
    // a quiet chip)
    // sub-group form (cond-only evaluations of a CFG-shaped run): x / eps hold x.n < n samples that start at index sample0 of the context
    // batch, and run on sub_lanes(x.n) of the configured lanes, in their arenas (planned by a dry pass of this form too)
    void forward(UNet& u, hipStream_t main_st, bool dry, bool concurrent, const Act& x, const Act& eps, const float* temb, const int* tidx,
                 const FwdOpt& o = FwdOpt());
    int sub_lanes(int n_sub) const { int g = G; while (g > 1 && (n_sub % g)) --g; return g; }   // the default rule: lowered until it divides
    void commit_plan();                     // after the dry pass: (re)allocate what grew; not capturable
    // part of the hipGraph key (GraphKey): lane count and every address a captured lane may touch, zero beyond G
    struct Key { int G; const void* arena[MAXG]; const void* stats[MAXG]; };
    void key(Key& k) const;
    ~UNetLanes();
};

struct VAECfg {
    int in_channels = 3, out_channels = 3, latent_channels = 4;
    int boc[4] = {128, 256, 512, 512};
    int layers_per_block = 2;
    int groups = 32;
    float scaling_factor = 0.18215f;
    float eps = 1e-6f;
};
struct VAEAttn { DNorm gn; DConv qk, v, proj; int C = 0; };
struct VAE {
    VAECfg cfg;
    DevPool pool;
    // encoder
    DConv e_conv_in, e_conv_out /* quant_conv folded in */; DNorm e_norm_out;
    std::vector<ResBlock> e_res; DConv e_down[3]; ResBlock e_mid[2]; VAEAttn e_attn;
    // decoder
    DConv d_conv_in, d_conv_out; DNorm d_norm_out; float pq_w[16]; float pq_b[4]; float* d_pq = nullptr;  // post_quant 4x4 on device
    std::vector<ResBlock> d_res; DConv d_up[3]; ResBlock d_mid[2]; VAEAttn d_attn;
    Arena arena; float* stats = nullptr; size_t stats_cap = 0;
    // fp16-range guard of the decoder (with the released weights the decoder's residual stream can exceed 65504).
    // The stream is stored multiplied by 2^-range_shift; GroupNorm is scale invariant (its eps is scaled by 4^-shift), every branch that
    // feeds the stream is scaled in its producer's epilogue, so the result is the same function with 2^shift more head-room.
    // range_shift < 0 = automatic: run at shift 0, and if a GroupNorm saw non-finite statistics (d_bad) re-run at 4, then 8.
    int range_shift = -1; int last_shift = 0; int* d_bad = nullptr;
    // attached range probe (not owned): encoder.conv_in / down_blocks.i / mid_block, quant_conv (moments), post_quant_conv,
    // decoder.mid_block / up_blocks.i / conv_out.  Decoder stream points are reported at their true scale (stored value x 2^shift) and
    // are what the stream holds, i.e. with the EMASC skip that the producing epilogue folds in
    Probe* probe = nullptr;

    void load(const VAECfg& c, const WeightStore& ws);
    // x: [n,H,W,64] padded NHWC image. Returns moments Act [n,h,w,8]; feats[0..4] = encoder features idx1..5 (views)
    Act encode(Ctx& c, const Act& x, Act feats[5]);
    // z: [n,h,w,64] padded NHWC (post_quant already applied); skips[0..4] = EMASC outputs for idx1..5 or null; shift: see range_shift
    Act decode(Ctx& c, const Act& z, const Act* skips, int shift = 0);
    // decode under the range guard: runs `body(shift)` (which must call decode(c, z, skips, shift) and emit the outputs) once, or again
    // with a larger shift when the overflow flag came back set; returns the shift that was used.  Synchronises the stream once.
    template <typename Body> int decode_guarded(hipStream_t st, Body&& body);
    bool overflowed(hipStream_t st);     // reads (and clears) d_bad; synchronises `st`
    // Deferred form of the guard for the fused pipeline (round 6; VERDICT r04 / r05: the run used to end in a D2H copy + hipStreamSynchronize of
    // the flag on every call).  A run decodes ONCE, at guard_shift(), and post_overflow_check() queues flag -> pinned host word, flag reset and
    // an event behind it: no host round trip.  poll_overflow() -- called at the entry of the next run and by ladi_tryon_poll_overflow() --
    // waits for that event (long complete by then), and if the flag was set raises the automatic shift (0 -> 4 -> 8) and reports 1: the
    // images of THAT run are invalid and the caller re-submits it (pipeline.py does so transparently when it hands out host results; with
    // device-resident results the next call fails loudly instead of returning garbage).
    int auto_shift = 0; int* h_bad = nullptr; hipEvent_t ev_bad = nullptr; bool bad_pending = false;
    int guard_shift() const { return range_shift >= 0 ? range_shift : auto_shift; }
    void post_overflow_check(hipStream_t st);
    int poll_overflow();                 // 0: nothing pending / last checked run was fine; 1: it overflowed (automatic shift raised if possible)
    ~VAE();
};

template <typename Body>
int VAE::decode_guarded(hipStream_t st, Body&& body) {
    const int fixed = range_shift;
    const int tries[3] = {0, 4, 8};
    for (int t = 0; t < 3; ++t) {
        const int sh = fixed >= 0 ? fixed : tries[t];
        body(sh);
        last_shift = sh;
        if (!overflowed(st)) return sh;
        if (fixed >= 0) break;
        if (probe) { probe->reset_prefix("decoder.", st); probe->reset_prefix("post_quant_conv", st); }   // the retry reports its own values
    }
    throw std::runtime_error("VAE decode: activations exceed the fp16 range (non-finite GroupNorm statistics) at range shift " +
                             std::to_string(last_shift));
}

struct EMASCCfg { int n = 5; int in_ch[8] = {128, 128, 128, 256, 512}; int out_ch[8] = {128, 256, 512, 512, 512}; };
struct EMASC {
    EMASCCfg cfg; DevPool pool; DConv a[8], b[8];
    Arena arena;
    Probe* probe = nullptr;                 // attached range probe (not owned): emasc.i = output i (after the mask)
    void load(const EMASCCfg& c, const WeightStore& ws);
    // out[i] = conv_b(silu(conv_a(feat[i]))) * (1 - mask[i])   (mask[i] may be null)
    void forward(Ctx& c, const Act* feats, const h16* const* masks, Act* outs, bool outs_preallocated = false);
};

struct AdapterCfg { int hidden = 1280, heads = 16, mlp = 5120, head_hidden = 5120, out_dim = 16384; float ln_eps = 1e-5f; };
struct Adapter {
    AdapterCfg cfg; DevPool pool;
    DNorm ln1, ln2, post_ln; DConv q, kv, o, fc1, fc2, l0, l3, l6;
    Arena arena;
    void load(const AdapterCfg& c, const WeightStore& ws);
    // x [B][T][hidden] fp16 dense -> out [B][out_dim] fp16
    int forward(const h16* x, int B, int T, h16* out, hipStream_t st);
};

// CLIP text encoder + pseudo-word splice (reference src/utils/encode_text_word_embedding.py:6-72)
struct TextCfg { int vocab = 49408, hidden = 1024, heads = 16, mlp = 4096, layers = 23, max_pos = 77, vstar_id = 259; float ln_eps = 1e-5f; };
struct TextLayer { DNorm ln1, ln2; DConv qkv, o, fc1, fc2; };   // one pre-LN CLIP encoder layer (text and vision towers)
std::vector<TextLayer> load_clip_layers(DevPool& pool, const WeightStore& ws, const std::string& prefix, int n);   // prefix + "<i>.layer_norm1" ...
// dst = cur + attn(LN1(cur)) -> + fc2(gelu(fc1(LN2(.)))) over tokens cur [B, T, 1, hidden]; head dim 64: flash kernel (causal or not), else the
// generic-head-dim kernel (non-causal); softmax scale 1 / sqrt(head dim).  dst: caller-owned view of cur's shape, not cur itself
void clip_layer(Ctx& c, const TextLayer& L, const Act& cur, Act& dst, int heads, bool causal, float eps);
struct TextEncoder {
    TextCfg cfg; DevPool pool;
    h16* tok = nullptr; h16* pos = nullptr;   // [vocab][hidden], [max_pos][hidden]
    std::vector<TextLayer> layers; DNorm final_ln;
    Arena arena;
    int* d_ids = nullptr; int ids_cap = 0;    // ids [B*T] | first [B] | eot row [B]
    int* h_meta = nullptr; int h_cap = 0; hipEvent_t h_done = nullptr;   // pinned staging of the host-id path + "copy has been consumed" event
    void load(const TextCfg& c, const WeightStore& ws);
    // ids [B][T] int32 on the host (validated, errors like the reference) or on the device (ids_on_device: no host round trip, no
    // validation -- out-of-range ids are clamped by the lookup, slots past the sequence end are cut); word_emb fp16 [B][nv][hidden]
    // (device) or null; out_hidden [B][T][hidden]; out_pooled [B][hidden] or null.  Asynchronous on `st` in both forms.
    int forward(const int* ids, int ids_on_device, int B, int T, const h16* word_emb, int nv, h16* out_hidden, h16* out_pooled, hipStream_t st);
    ~TextEncoder();
};

// CLIP ViT-H/14 vision encoder (the `vision_encoder(pixel_values).last_hidden_state` of src/inference.py:269-273)
struct VisionCfg { int hidden = 1280, heads = 16, mlp = 5120, layers = 32, image = 224, patch = 14; float ln_eps = 1e-5f; };
struct VisionEncoder {
    VisionCfg cfg; DevPool pool;
    DConv patch;                 // [hidden][3*ps*ps padded to 64] bias-free
    h16* posc = nullptr;         // [tokens][hidden]: position embedding, class embedding added to row 0
    DNorm pre_ln, post_ln; std::vector<TextLayer> layers;
    h16* vproj = nullptr; int proj_dim = 0;   // visual_projection.weight [proj_dim][hidden], bias-free (CLIPVisionModelWithProjection); 0: not in the weights
    Arena arena;
    int tokens() const { return 1 + (cfg.image / cfg.patch) * (cfg.image / cfg.patch); }
    void load(const VisionCfg& c, const WeightStore& ws);
    // pixels [B][3][image][image] (fp32 or fp16, device); out_hidden fp16 [B][tokens][hidden] (encoder output, no post_layernorm);
    // out_pooled fp16 [B][hidden] = post_layernorm(out_hidden[:, 0]) or null
    int forward(const void* pixels, int in_f32, int B, h16* out_hidden, h16* out_pooled, hipStream_t st);
    // the same with every output optional (null: not produced; what a missing output's readers need lives in the arena), plus out_penultimate fp16 [B][tokens][hidden] = the input of the last encoder layer (hidden_states[-2]; with one layer
    // the pre_layrnorm output), written by its producer directly, and out_image_embeds fp16 [B][proj_dim] = visual_projection(pooled).
    // out_image_embeds without a loaded projection is refused before anything is launched.  Shared outputs are forward()'s bit for bit
    int forward_ex(const void* pixels, int in_f32, int B, h16* out_hidden, h16* out_pooled, h16* out_penultimate, h16* out_image_embeds,
                   hipStream_t st);
};

// ---- fp32 path of the warping module (runtime_f32.cpp, f32path.hip): src/inference.py:253,264 call both networks on fp32 tensors
struct ActF { float* p = nullptr; int n = 0, h = 0, w = 0, c = 0, ld = 0; size_t pixels() const { return (size_t)n * h * w; } };
struct DConvF {   // fp32 weights [cout][k*k][cin_pad] (cin padded to a multiple of 8), fp32 bias or null
    float* w = nullptr; float* b = nullptr;
    int cin = 0, cin_pad = 0, cout = 0, k = 1;
    int K() const { return k * k * cin_pad; }
};
DConvF load_conv_f32(DevPool& pool, const HostTensor& w, const HostTensor* bias);
ActF new_act_f32(Ctx& c, int n, int h, int w, int cc);
ActF conv2d_f32(Ctx& c, const DConvF& cv, const ActF& x, const ActF* x2, int stride, int pad, int act);
// conv (+ optional own bias) followed by an inference-mode BatchNorm, folded on the host in fp32: w' = w * s, b' = (b - mean) * s + beta
void fold_conv_bn(const WeightStore& ws, const std::string& conv, const std::string& bn, float eps, HostTensor& fw, HostTensor& fb);

// Refinement UNet of the warping module (first half): src/models/UNet.py UNetVanilla(24, 3, bilinear=True) as
// instantiated by hubconf.py:57 and called at src/inference.py:264.  BatchNorm (inference mode) is folded into the bias-free convs.
struct RefineCfg { int in_ch = 24, out_ch = 3, base = 64; float bn_eps = 1e-5f; };
struct DoubleConvW { DConv c1, c2; };
struct DoubleConvWF { DConvF c1, c2; };
struct Refine {
    RefineCfg cfg; DevPool pool;
    DoubleConvW inc, down[4], up[4]; DConv outc;
    DoubleConvWF incf, downf[4], upf[4]; DConvF outcf;      // fp32 copies (fp32 callers)
    Arena arena;
    void load(const RefineCfg& c, const WeightStore& ws);
    // x [B, in_ch, H, W] NCHW fp32/fp16 (device) -> out [B, out_ch, H, W] NCHW fp32/fp16; H, W multiples of 16.  fp32 input runs the
    // network in fp32 (weights, activations, accumulation: inference.py:264), fp16 input in fp16 storage / fp32 accumulation
    int forward(const void* x, int in_f32, int B, int H, int W, void* out, int out_f32, hipStream_t st);
    int forward_f32(const void* x, int B, int H, int W, void* out, int out_f32, hipStream_t st);
};

// TPS geometric-matching network of the warping module (second half): src/models/ConvNet_TPS.py ConvNet_TPS as
// instantiated by hubconf.py:56 (256x192, input_nc = 21, n_layer = 3) and called at src/inference.py:253
struct TpsCfg { int height = 256, width = 192, input_nc = 21, n_layers = 3, grid = 5, ngf = 64; float bn_eps = 1e-5f; };
struct TpsExtract { std::vector<DConv> conv; std::vector<float*> bn_scale, bn_shift; };   // conv i -> ReLU -> (BatchNorm i, except after the last)
struct TpsExtractF { std::vector<DConvF> conv; };
struct Tps {
    TpsCfg cfg; DevPool pool;
    TpsExtract ea, eb;
    DConv reg[4]; DConv lin;          // regression convs (BatchNorm folded) and the control-point linear (columns permuted to NHWC order)
    TpsExtractF eaf, ebf; DConvF regf[4]; float* linf_w = nullptr; float* linf_b = nullptr;   // fp32 copies (fp32 callers; bn_scale / bn_shift shared)
    int forward_f32(const void* a, const void* b, int B, float* grid, float* coor, hipStream_t st);
    float* d_inv = nullptr; float* d_ctrl = nullptr;   // TPSGridGen inverse kernel [(N+3)^2], target control points [N][2]
    int* d_perm = nullptr; int perm_cap = 0;           // correlation row order of feature A (column-major positions)
    Arena arena;
    void load(const TpsCfg& c, const WeightStore& ws);
    // a [B,3,H,W], b [B,input_nc,H,W] NCHW fp32/fp16 (device) -> grid [B,H,W,2] fp32, coor [B,grid*grid,2] fp32 (or null)
    int forward(const void* a, const void* b, int in_f32, int B, float* grid, float* coor, hipStream_t st);
    ~Tps();
};

struct TryOnInputs {
    int batch, height, width, in_f32;
    const void *image, *mask_image, *pose_map, *warped_cloth;
    int pose_channels;
    const h16 *prompt_embeds, *negative_prompt_embeds; int L;
    const float *noise_cloth, *noise_latents, *noise_masked;
    int steps; float guidance; int scheduler; int cloth_zero_from; int no_pose; int use_graph;
    const float* alphas_cumprod;  // optional [1000] host
};
enum { TRYON_PAG_WITH_CACHE = -12 };  // TryOn::run: a PAG table with a positive entry together with a feature-cache plan (LADI_TRYON_PAG_WITH_FEATURE_CACHE)
enum { TRYON_IP_NO_ADAPTER = -13 };   // TryOn::run: image embeddings are set but the UNet has no IP-Adapter loaded (LADI_TRYON_IP_NO_ADAPTER)
// TryOn::run: embeddings [B][E] are set but the loaded adapter is a Plus adapter, or hidden states [B][T][E] but it is a plain one
enum { TRYON_IP_ADAPTER_KIND = -19 };
// TryOn::run with self-attention guidance on (ladi_tryon_set_sag), refused before anything is launched (LADI_TRYON_SAG_*):
enum {
    TRYON_SAG_WITH_CACHE = -14,    // together with a feature-cache plan: shallow evaluations do not run the mid block
    TRYON_SAG_WITH_PAG = -15,      // together with a positive PAG scale
    TRYON_SAG_TOME_MID = -16,      // token merging configured so that the mid block merges
    TRYON_SAG_SCHEDULER = -17,     // a sigma-space scheduler (Euler, Euler-ancestral, LMS)
    TRYON_SAG_SMALL = -18          // latents under 5 x 5 (the blur's reflect padding)
};
enum { TRYON_CALLBACK_ABORT = -8 };   // TryOn::run: the step callback returned non-zero (LADI_TRYON_CALLBACK_ABORTED, include/ladi_native.h)
// The forms of one evaluation of the fused loop: bit 0 cond-only, bit 1 shallow (feature cache), bit 2 PAG (never together with bit 1), so
// 0 .. 5.  The form is the index of GraphTable and of EvalPlan::has_form.

// The captured graphs of one owner, one slot per form
struct GraphTable {
    static constexpr int N = 6;
    hipGraph_t g[N] = {}; hipGraphExec_t e[N] = {};
    long long captures = 0;  // captures made over the owner's life (ladi_tryon_graph_captures): a run that replays what it has adds none
    void clear();            // destroy every graph and executable (the owner's destructor; a changed GraphKey)
    // capture fn's launches on st into slot f and instantiate them; a throw of fn ends the capture and is passed on.  A graph left in the slot
    // by a capture whose instantiation failed is destroyed first
    void capture(int f, hipStream_t st, const std::function<void()>& fn);
};
// What the captured graphs of a TryOn were captured with.  The rule: a value that a captured launch carries as an argument, or a pointer it
// dereferences, is a field here.  Zeroed with memset before it is filled (so padding compares equal) and compared with memcmp: another key
// drops every graph.  A field that means something only with a feature on is zero when it is off
struct GraphKey {
    const void* arena;                          // base of the run's activation arena: every transient address
    int B, H, W, cfg, L, pose_ch, has_cloth;    // the shapes of every launch
    unsigned guidance;                          // bits of the scalar guidance, when !guided (with a table the scalar is ignored: zero)
    const void *d_table, *stats;
    const void *trace_eps, *trace_lat; int trace_cap;
    const void* step_noise;
    UNetLanes::Key lanes;
    // what the forward itself carries and dereferences: time-embedding table, cross-attention K/V, probe, FreeU, the PAG layers of a run with
    // perturbed samples, the image context, token merging (UNet::key)
    UNet::Key unet;
    // every form lives under one key, with the guidance table, the factor buffer and phi (its bits, when guided)
    const void *guidance_tab, *factor; int guided; unsigned phi;
    // ... and with the feature cache: its buffer, the branch and whether whole evaluations capture (a graph captured with capture on is never
    // replayed for a plain run, nor the reverse); buffer and branch when fc_on
    const void* fcache; int fc_on, fc_branch;
    // ... and with the latent blend: its buffers, the coefficient table and the mode (when the latents bit is set)
    const void *keep_x0, *keep_noise, *keep_mask, *keep_tab; int preserve_mode;
    // ... and with PAG: whether the run has the third group and its scale table; a graph captured with PAG is never replayed without it,
    // nor the reverse
    int pag_on; const void* pag_tab;
    // ... and with SAG: whether every evaluation has the degrade launch and the second forward, the device scale and the alpha table.  The
    // scale's VALUE is not part of the key: the graphs read it from device memory
    int sag_on; const void *sag_scale, *sag_tab;
};
// The per-evaluation plan of one run: host arithmetic only (plan_evals; ladi_tryon_plan_forms runs it without a GPU)
struct EvalPlan {
    bool cfg = false;          // CFG-shaped: ANY evaluation's scale is > 1 (a set schedule replaces the scalar)
    bool guided = false;       // the scales come from a device table (a schedule, or the scalar repeated for the rescale statistics)
    bool use_factor = false;   // guided with phi > 0: the rescale statistics run
    bool pag_on = false;       // PAG-shaped (a third sample group): ANY PAG scale is > 0
    bool fc_on = false;        // some evaluation runs shallow, after promotion; else the plain run: capture stays off
    int ng = 1, groups = 1;    // sample groups of a plain evaluation ([uncond ; cond] or [cond]); of the run: ng + pag_on
    std::vector<float> gtab;   // scale of every evaluation
    std::vector<unsigned char> form;   // form of every evaluation, after the feature cache's one promotion
    bool has_form[GraphTable::N] = {};
    bool sag_on = false;       // SAG run: EVERY evaluation degrades and runs a second forward over B samples; the forms are the plain run's
    int rc = 0; std::string error;     // a refusal: -9 (guidance / PAG table length), -10 (feature-cache plan), TRYON_PAG_WITH_CACHE, TRYON_SAG_*
};
// What plan_evals needs to know of a run with self-attention guidance (scale != 0 = on): the scheduler code, the latent size and whether the
// UNet's token merging merges in the mid block
struct SagPlan { float scale = 0.f; int scheduler = 0, h = 0, w = 0; bool mid_merges = false; };
// first_step / steps: for the message of a length refusal only.  Returns p.rc
int plan_evals(EvalPlan& p, int evals, int first_step, int steps, float guidance, const std::vector<float>& g_sched, float phi,
               const std::vector<float>& pag_sched, const std::vector<unsigned char>& fc_plan, const SagPlan* sag = nullptr);

struct TryOn {
    UNet* unet = nullptr; VAE* vae = nullptr; EMASC* emasc = nullptr;
    Arena arena; float* stats = nullptr; size_t stats_cap = 0;
    DevPool pool;  // small persistent things
    StepTable* d_table = nullptr; int table_cap = 0; int* d_step = nullptr;
    int* sk_cnt = nullptr;   // split-K arrival counters of this handle's stream (Ctx::sk_cnt)
    // the captured evaluation of every form, and what they were captured with (all bytes zero, padding included, until the first capture)
    GraphTable graphs; GraphKey graph_key;
    TryOn() { std::memset(&graph_key, 0, sizeof(graph_key)); }
    UNetLanes lanes; int lanes_override = 0;   // sample-group lanes of the denoising loop (0 = LADI_UNET_LANES / default)
    hipEvent_t ev[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr}; bool ev_valid = false;
    int last_evals = 0;
    float* trace_eps = nullptr; float* trace_lat = nullptr; int trace_cap = 0;   // caller-owned per-evaluation trace buffers (tests)
    // step noise (Euler-ancestral, DDIM with eta > 0): the caller's fp32 [steps][B][4][h][w] (ladi_tryon_set_step_noise), copied by run() into the
    // runtime-owned step_noise_buf that the captured graph reads
    const float* step_noise_src = nullptr; int step_noise_steps = 0;
    float* step_noise_buf = nullptr; size_t step_noise_cap = 0;
    float eta = 0.f;   // DDIM's eta / TCD's gamma (ladi_tryon_set_eta), sticky; other kinds refuse a non-zero one
    // start from given latents at step init_first of the schedule (ladi_tryon_set_init, sticky; null or init_first = 0: off): the caller's fp32
    // NCHW [B][4][init_hs][init_ws], read once by init_latents_kernel on the run's stream before the loop (never inside the captured graph),
    // which resamples it to the run's latent size and mixes it with noise_latents (init_noisy: taken as the loop's latents unchanged)
    const float* init_src = nullptr; int init_hs = 0, init_ws = 0, init_first = 0, init_noisy = 0;
    // per-evaluation guidance (ladi_tryon_set_guidance_schedule, sticky; empty = in.guidance for every evaluation) and guidance rescale phi
    // (ladi_tryon_set_guidance_rescale).  A run is CFG-shaped (2B rows, both contexts) if any scale is > 1; inside such a run an evaluation
    // whose scale is <= 1 runs the UNet over the conditional samples [B, 2B) only (form bit 0).  With a schedule or phi > 0 the scales come
    // from the device table d_gtab, so the graphs of the full and of the cond-only form serve every value
    std::vector<float> g_sched; float phi = 0.f;
    float* d_gtab = nullptr; int gtab_cap = 0; float* d_factor = nullptr; int factor_cap = 0;
    int last_cond_only = 0;   // evaluations of the last run that ran cond-only (ladi_tryon_cond_only_evals)
    // deep-feature cache (ladi_tryon_set_feature_cache, sticky; empty plan = off): fc_plan holds one flag per evaluation, 1 = whole forward
    // (which captures into fcache), 0 = shallow forward from fcache at fc_branch (form bit 1).  fcache is persistent (outside the
    // per-evaluation arena region) and grow-only: fp16 [n][h][w][fc_channels]
    std::vector<unsigned char> fc_plan; int fc_branch = 0;
    h16* fcache = nullptr; size_t fcache_cap = 0;
    // perturbed-attention guidance (ladi_tryon_set_pag, sticky; empty = off: nothing below is allocated or launched): one scale per
    // evaluation.  With any scale > 0 the run is PAG-shaped: unet_in, eps and the context grow by a third group of B samples behind the
    // cond group ([uncond ; cond ; perturbed], or [cond ; perturbed] without CFG), the scales go to the device table d_pag, and an evaluation
    // with a scale > 0 runs the forward over the perturbed group too (form bit 2; never together with the feature cache, which run() refuses)
    std::vector<float> pag_sched;
    float* d_pag = nullptr; int pag_cap = 0;
    // self-attention guidance (ladi_tryon_set_sag, sticky; 0 = off: nothing below is allocated or launched).  On: unet_in and eps grow by
    // one group of B rows behind the last (the context does not), and every evaluation is first forward (capturing the SAG map) ->
    // sag_degrade into those rows -> second forward over them with the base group's context rows -> combine + step.  The scale lives in the
    // device word d_sag (uploaded per run: another value replays the same graphs); d_sag_tab holds {sqrt(a), sqrt(1 - a), 1, 0} per evaluation
    float sag_scale = 0.f;
    float* d_sag = nullptr; float* d_sag_tab = nullptr; int sag_tab_cap = 0;
    // image prompt (ladi_tryon_set_ip_adapter, sticky; ip_pos null = off: the run clears the UNet's image context and launches the plain
    // run).  The caller's fp16 [B][E] embeddings (ip_neg null: zeros, diffusers' zeros_like) are assembled per run into the runtime-owned
    // ip_buf [groups * B][E] -- [neg ; pos], [neg ; pos ; pos] with PAG, [pos] without CFG -- on the run's stream, next to the prompt
    // embeddings, and become the UNet's image context right after set_context
    // ladi_tryon_set_ip_adapter_seq (the two setters replace each other): ip_T > 0, the pointers are hidden states fp16 [B][ip_T][E] of a
    // Plus adapter, the rows assembled are ip_T * E halves wide and go through UNet::set_ip_context_seq (the Resampler); ip_T = 0: embeddings
    const h16* ip_pos = nullptr; const h16* ip_neg = nullptr; int ip_T = 0;
    h16* ip_buf = nullptr; size_t ip_buf_cap = 0;
    int last_shallow = 0;     // evaluations of the last run that ran shallow, after promotion (ladi_tryon_shallow_evals)
    // preserve-unmasked (ladi_tryon_set_preserve, sticky; 0 = off: nothing below is allocated or launched).  Bit 0, latents: after every
    // scheduler update the keep pixels (1 - maxpool8x8 of the binarised mask) become k_x z0 + k_n noise at the next timestep, z0 = scaling *
    // mode(encode(image)); z0, the noise (a copy of noise_latents) and the keep mask live in the persistent part of the arena, the
    // coefficients in d_keep_tab, so a captured graph holds no caller pointer.  Bit 1, pixels: the decode epilogue composites the decoded
    // image over the input image with the binarised mask, blurred with a Gaussian of preserve_sigma pixels when that is > 0
    int preserve_mode = 0; float preserve_sigma = 0.f;
    float* d_keep_tab = nullptr; int keep_tab_cap = 0;
    // step callback (ladi_tryon_set_step_callback): after evaluation i with i % cb_every == 0 the latents go to the caller's fp32 NCHW
    // cb_latents, cb_fn(cb_user, i) runs on the host, and cb_latents comes back (edits included); fn == null = off
    int (*cb_fn)(void*, int) = nullptr; void* cb_user = nullptr; int cb_every = 1; float* cb_latents = nullptr;
    // the legacy NULL stream (torch's default) cannot be captured: work then runs on this internal stream, fenced
    // against the caller's stream with events on entry and exit
    hipStream_t own_stream = nullptr; hipEvent_t ev_in = nullptr, ev_out = nullptr;
    // stage times of the last run (ms): [0] preprocess+VAE encodes+EMASC, [1] denoising loop, [2] decode ; call after a sync
    int stage_ms(float out[3]);
    // images_out: fp32 [B,H,W,3] in [0,1], or (images_u8) uint8 = round(image * 255)
    int run(const TryOnInputs& in, void* images_out, int images_u8, float* latents_out, hipStream_t st);
    // the stages of run(), in its order, over the state of one run (runtime_tryon.cpp).  The int ones return a refusal code or 0
    struct Run;
    int enter(Run& r);              // stream fence, overflow poll
    int plan(Run& r);               // geometry, scheduler tables (host), evaluation plan
    int grow_tables(Run& r);        // grow-only device tables, step-noise buffer, events; last of all the feature cache
    void upload_tables(Run& r);     // real pass: probes from zero, the tables' uploads, time embeddings (r.rc = -5)
    void encode(Run& r);            // persistent buffers, preprocessing and VAE encodes, static UNet input (r.rc = -6)
    void denoise(Run& r);           // the loop: eager, or graph replay by form; the callback point (r.cb_rc)
    void decode(Run& r);            // VAE decode, composite, outputs
    ~TryOn();
};

// scheduler tables (host): builds timesteps + StepTable entries. kind 0 = DDIM, 1 = PNDM(PLMS, skip_prk_steps), 2 = LMSDiscrete
// (fractional timesteps, sigma parameterisation: the latents start at noise * init_noise_sigma and the UNet sees them scaled),
// 3 = DPMSolverMultistep (dpmsolver++), 4 = EulerDiscrete, 5 = EulerAncestralDiscrete (LMS's timesteps and sigmas).
// The scheduler code (ladi_tryon_inputs.scheduler, include/ladi_native.h) carries the kind in bits 0-3 and the DPM-Solver++ options in
// bits 8-11: bits 8-9 solver_order (0 = the default 2, else 1..3), bit 10 solver_type heun (0 = midpoint), bit 11 lower_order_final off.
// 7 = LCM and 8 = TCD (few-step sampling of distilled weights; kinds 6, 9 and 15 stay unknown).  Bit 6: trailing timestep spacing (DDIM, Euler
// and Euler-ancestral only); bits 12-21: original_inference_steps of LCM / TCD (1..1000, 0 = 50; those two kinds only).
// Any other bit, an option bit on another kind, or an unknown kind is rejected.
enum { SCHED_DDIM = 0, SCHED_PNDM = 1, SCHED_LMS = 2, SCHED_DPMPP = 3, SCHED_EULER = 4, SCHED_EULER_A = 5, SCHED_LCM = 7, SCHED_TCD = 8 };
struct SchedCode { int kind = 0, order = 2, heun = 0, lower_order_final = 1, trailing = 0, original_steps = 50; };
SchedCode decode_sched_code(int code);
void default_alphas_cumprod(std::vector<float>& ac);
struct SchedInfo {
    float init_noise_sigma = 1.f;    // prepare_latents: latents = noise * init_noise_sigma (tryon_pipe.py:424)
    float in_scale0 = 1.f;           // scale_model_input of the run's first evaluation (later evaluations: StepTable::in_scale_next)
    std::vector<float> sigmas;       // LMS / Euler / Euler-ancestral: steps + 1 values (trailing 0), the whole schedule whatever first_step
    std::vector<float> lms_coeffs;   // LMS only: [steps][4], c_ij over [d_i, d_{i-1}, d_{i-2}, d_{i-3}] (rows before first_step stay 0)
    // start latents of a run that begins at step first_step > 0: x = start_kx * init + start_kn * noise (double arithmetic, held in fp32).
    // DDIM / PNDM / DPM-Solver++: sqrt(a_t), sqrt(1 - a_t) at t = timesteps[first_step]; LMS / Euler / Euler-ancestral: 1, sigma[first_step].
    // first_step = 0: {0, init_noise_sigma}, i.e. today's latents = noise * init_noise_sigma
    float start_kx = 0.f, start_kn = 1.f;
};
// cloth_zero_from: first evaluation index that must see zero cloth latents (tryon_pipe.py:718), computed by the caller in float64;
// code: the scheduler code above; eta: DDIMScheduler.step's eta (>= 0; > 0 puts the stochastic term into c_n) or TCDScheduler.step's gamma
// ([0, 1]; > 0 re-noises every update but the last); a non-zero eta with any other kind is refused.
// Step counts: [2, 1000] for the plain codes 0-5, [1, 1000] with the trailing bit, [1, original_inference_steps] for LCM / TCD.
// first_step > 0 builds the tail of the `steps`-step schedule (strength): the evaluations of steps first_step .. with their own timesteps and
// sigmas, indexed from 0 (cloth_zero_from too).  Multistep history starts empty there: LMS and DPM-Solver++ warm up again (orders 1, 2, ..),
// lower_order_final acts where it does in the whole run, and PNDM restarts as a fresh PLMS run over the tail's step timesteps u0 > u1 > ..
// (evaluations [u0, u1, u1, u2, ..]: tail steps + 1; not diffusers' slice of the N + 1 list, which leaves the sample one step
// under-denoised).  first_step <= steps - 1 (PNDM: steps - 2); first_step = 0 gives the whole run's tables bit for bit.
void build_step_table(int code, int steps, const float* alphas_cumprod, int cloth_zero_from, std::vector<double>& timesteps,
                      std::vector<StepTable>& table, SchedInfo* info = nullptr, double eta = 0.0, int first_step = 0);
// preserve-unmasked latent blend: out[i] = {k_x, k_n} of the scheduler's add_noise at timesteps[i + 1], the timestep the latents belong to
// after the update of evaluation i (DDIM / PNDM / DPM-Solver++: sqrt(a), sqrt(1 - a); LMS / Euler / Euler-ancestral: 1, sigma[i + 1]), float64
// arithmetic held in fp32; the last row is {1, 0}.  For a whole run or a tail (first_step), one row per evaluation of build_step_table
void build_keep_coeffs(int code, int steps, const float* alphas_cumprod, int first_step, std::vector<float>& out);
// the same from the timesteps and SchedInfo a build_step_table(code, .., first_step) call returned
void keep_coeffs_of(int code, const std::vector<double>& timesteps, const SchedInfo& info, const float* alphas_cumprod, int first_step,
                    std::vector<float>& out);
// true if the table has a stochastic term (some c_n != 0: Euler-ancestral, DDIM with eta > 0, LCM and TCD with eta > 0 of more than one
// evaluation), i.e. a run of it needs step noise
bool table_needs_step_noise(const std::vector<StepTable>& table);

}  // namespace ladi
