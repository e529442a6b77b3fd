// IP-Adapter Plus image projection: the `Resampler` of tencent-ailab/IP-Adapter (a Perceiver resampler), which turns the hidden states of
// an image encoder into N image tokens.  Restated from memory of that package -- it is not a dependency and was not checked against it:
//
//     lat = latents.expand(n)                                  parameter [1, N, dim]
//     x   = proj_in(x)                                         Linear E -> dim, bias
//     for every layer:
//         xn, ln = LayerNorm(norm1)(x), LayerNorm(norm2)(lat)
//         q = to_q(ln);  k, v = to_kv(cat([xn, ln], tokens)).chunk(2, -1)          no biases; T + N keys
//         a = softmax((q s) (k s)^T) v per head, s = dim_head^-0.25                 = logits / sqrt(dim_head), softmax in fp32
//         lat = to_out(a) + lat                                                    no bias
//         lat = W2(gelu(W1(LayerNorm(lat)))) + lat                                 dim -> 4 dim -> dim, no biases, erf GELU
//     tokens = LayerNorm(norm_out)(proj_out(lat))                                  Linear dim -> out_dim, bias
//
// every LayerNorm with eps 1e-5.  Runs once per call, outside the denoising loop, and is built from the kernels of the hot path: igemm
// (small_linear for a width that is no multiple of 32), layer_norm_ld, flash_attn64 / attn_generic and the GELU epilogue.  LayerNorm(norm1)
// writes each sample's T rows straight into one [T + N]-row buffer per sample (one launch per sample: the launcher takes one row stride);
// LayerNorm(norm2)(lat) runs once, dense, for to_q, and one strided device copy puts its N rows per sample behind them, so to_kv is one GEMM.
#include "runtime.h"
#include <cmath>
#include <cstring>
#include <stdexcept>
#include <utility>

namespace ladi {

#define HIP_OK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) throw std::runtime_error(std::string(#x) + ": " + hipGetErrorString(e_)); } while (0)

namespace {

std::string shape_str(const HostTensor& t) {
    std::string s = "[";
    for (size_t i = 0; i < t.shape.size(); ++i) s += (i ? ", " : "") + std::to_string(t.shape[i]);
    return s + "]";
}

// Linear weight [cout][cin] as it is: the rows are not padded (cin % 8 == 0 is the caller's check), so igemm reads it with K = cin and
// small_linear with the same pointer
DConv upload_linear(DevPool& pool, const HostTensor& w, const HostTensor* bias) {
    DConv d; d.k = 1; d.cout = (int)w.shape[0]; d.cin = d.cin_pad = (int)w.shape[1];
    d.w = pool.upload_h16(w.data);
    if (bias) d.b = pool.upload_h16(bias->data);
    return d;
}

Act rows_view(h16* p, int rows, int c) {
    Act a; a.p = p; a.n = 1; a.h = rows; a.w = 1; a.c = c; a.ld = c;
    return a;
}

// dst [rows][cout] = act(x [rows][cin] W^T + bias) (+ res): igemm, or small_linear where igemm's 32-channel granularity does not hold
void linear(Ctx& c, const DConv& cv, const Act& x, Act& dst, int act, const Act* res) {
    if (cv.cin % 32 == 0) {
        ConvOpt o; o.act = act; o.res0 = res; o.dst = &dst;
        (void)conv2d(c, cv, x, nullptr, o);
        return;
    }
    if (c.dry()) return;
    c.check(ladi_launch_small_linear(x.p, 0, x.ld, cv.w, cv.b, res ? res->p : nullptr, res ? res->ld : 0, (int)x.pixels(), cv.cout, cv.cin, act, 0,
                                     dst.p, 0, dst.ld, c.st), "small_linear");
}

}  // namespace

void Resampler::check(const WeightStore& ws, const std::string& pre, int dh) {
    auto need = [&](const std::string& k) -> const HostTensor& {
        if (!ws.has(pre + k)) throw std::runtime_error("Resampler: '" + pre + k + "' is missing");
        return ws.get(pre + k);
    };
    auto mat = [&](const std::string& k, long long rows, long long cols) -> const HostTensor& {
        const HostTensor& t = need(k);
        if (t.shape.size() != 2 || (rows >= 0 && t.shape[0] != rows) || (cols >= 0 && t.shape[1] != cols) || t.shape[0] < 1 || t.shape[1] < 1)
            throw std::runtime_error("Resampler: " + pre + k + " of shape " + shape_str(t) + " is not [" + (rows >= 0 ? std::to_string(rows) : "*") + ", " +
                                     (cols >= 0 ? std::to_string(cols) : "*") + "]");
        return t;
    };
    auto vec = [&](const std::string& k, long long len) {
        if ((long long)need(k).numel() != len) throw std::runtime_error("Resampler: " + pre + k + " does not have " + std::to_string(len) + " entries");
    };
    // ---- geometry and every shape, before anything is uploaded
    if (!(dh == 64 || dh == 80 || dh == 96 || dh == 128))
        throw std::runtime_error("Resampler: dim_head " + std::to_string(dh) + " is not one of 64, 80, 96, 128");
    const HostTensor& lt = need("latents");
    if (lt.shape.size() != 3 || lt.shape[0] != 1 || lt.shape[1] < 1 || lt.shape[2] < 1)
        throw std::runtime_error("Resampler: " + pre + "latents of shape " + shape_str(lt) + " is not [1, N, dim]");
    const long long N_ = lt.shape[1], dim_ = lt.shape[2];
    if (N_ > 64) throw std::runtime_error("Resampler: " + std::to_string(N_) + " latents (image tokens), outside [1, 64]");
    const long long E_ = mat("proj_in.weight", dim_, -1).shape[1];
    vec("proj_in.bias", dim_);
    const long long out_ = mat("proj_out.weight", -1, dim_).shape[0];
    vec("proj_out.bias", out_); vec("norm_out.weight", out_); vec("norm_out.bias", out_);
    if (E_ % 8 || dim_ % 8 || out_ % 8)
        throw std::runtime_error("Resampler: the widths E = " + std::to_string(E_) + ", dim = " + std::to_string(dim_) + ", out_dim = " + std::to_string(out_) +
                                 " have to be multiples of 8");
    if (dim_ > 4096 || out_ > 4096) throw std::runtime_error("Resampler: dim and out_dim are limited to 4096 (LayerNorm)");
    int depth_ = 0;
    while (ws.has(pre + "layers." + std::to_string(depth_) + ".0.to_q.weight")) ++depth_;
    if (depth_ < 1) throw std::runtime_error("Resampler: '" + pre + "layers.0.0.to_q.weight' is missing (depth >= 1)");
    const long long inner = mat("layers.0.0.to_q.weight", -1, dim_).shape[0];
    if (inner % dh)
        throw std::runtime_error("Resampler: the attention width " + std::to_string(inner) + " is no multiple of dim_head " + std::to_string(dh));
    size_t expected = 7;
    for (int i = 0; i < depth_; ++i) {
        const std::string l = "layers." + std::to_string(i);
        for (const char* nm : {".0.norm1", ".0.norm2", ".1.0"}) { vec(l + nm + ".weight", dim_); vec(l + nm + ".bias", dim_); }
        mat(l + ".0.to_q.weight", inner, dim_); mat(l + ".0.to_kv.weight", 2 * inner, dim_); mat(l + ".0.to_out.weight", dim_, inner);
        const long long ff = mat(l + ".1.1.weight", -1, dim_).shape[0];
        if (ff % 8) throw std::runtime_error("Resampler: the feed-forward width " + std::to_string(ff) + " is no multiple of 8");
        mat(l + ".1.3.weight", dim_, ff);
        expected += 11;
    }
    size_t have = 0;
    for (auto& kv : ws.m) have += kv.first.compare(0, pre.size(), pre) == 0 && kv.first.size() > pre.size();
    if (have != expected) {
        // name the first key nobody reads: a bias on a bias-free Linear, a layer past a gap, another module's key
        for (auto& kv : ws.m) {
            const std::string& k = kv.first;
            if (k.compare(0, pre.size(), pre)) continue;
            const std::string r = k.substr(pre.size());
            bool known = r == "latents" || r == "proj_in.weight" || r == "proj_in.bias" || r == "proj_out.weight" || r == "proj_out.bias" ||
                         r == "norm_out.weight" || r == "norm_out.bias";
            for (int i = 0; i < depth_ && !known; ++i) {
                const std::string l = "layers." + std::to_string(i);
                for (const char* nm : {".0.norm1.weight", ".0.norm1.bias", ".0.norm2.weight", ".0.norm2.bias", ".0.to_q.weight", ".0.to_kv.weight",
                                       ".0.to_out.weight", ".1.0.weight", ".1.0.bias", ".1.1.weight", ".1.3.weight"})
                    known = known || r == l + nm;
            }
            if (!known) throw std::runtime_error("Resampler: unexpected key '" + k + "'");
        }
    }
    N = (int)N_; E = (int)E_; dim = (int)dim_; depth = depth_; dim_head = dh; heads = (int)(inner / dh); out_dim = (int)out_;
}

void Resampler::upload(const WeightStore& ws, const std::string& pre) {
    latents = pool.upload_h16(ws.get(pre + "latents").data);
    proj_in = upload_linear(pool, ws.get(pre + "proj_in.weight"), &ws.get(pre + "proj_in.bias"));
    proj_out = upload_linear(pool, ws.get(pre + "proj_out.weight"), &ws.get(pre + "proj_out.bias"));
    norm_out = load_norm(pool, ws, pre + "norm_out");
    layers.resize(depth);
    for (int i = 0; i < depth; ++i) {
        const std::string l = pre + "layers." + std::to_string(i);
        ResamplerLayer& L = layers[i];
        L.n1 = load_norm(pool, ws, l + ".0.norm1"); L.n2 = load_norm(pool, ws, l + ".0.norm2"); L.ffn = load_norm(pool, ws, l + ".1.0");
        L.q = upload_linear(pool, ws.get(l + ".0.to_q.weight"), nullptr);
        L.kv = upload_linear(pool, ws.get(l + ".0.to_kv.weight"), nullptr);
        L.o = upload_linear(pool, ws.get(l + ".0.to_out.weight"), nullptr);
        L.w1 = upload_linear(pool, ws.get(l + ".1.1.weight"), nullptr);
        L.w2 = upload_linear(pool, ws.get(l + ".1.3.weight"), nullptr);
    }
}

void Resampler::forward(const h16* x, int n, int T, h16* tokens_out, hipStream_t st) {
    if (!x || !tokens_out) throw std::runtime_error("Resampler: null input or output");
    if (n < 1 || T < 1) throw std::runtime_error("Resampler: " + std::to_string(n) + " samples of " + std::to_string(T) + " tokens: both have to be >= 1");
    const int inner = heads * dim_head, Nk = T + N;
    const float eps = 1e-5f;
    run_planned(arena, st, [&](Ctx& c) {
        Act xin = rows_view(const_cast<h16*>(x), n * T, E);
        Act xp = c.new_act(1, n * T, 1, dim);                                   // proj_in(x)
        Act la = c.new_act(1, n * N, 1, dim), lb = c.new_act(1, n * N, 1, dim);  // the latents, ping-pong
        linear(c, proj_in, xin, xp, LADI_ACT_NONE, nullptr);
        if (!c.dry())
            for (int s = 0; s < n; ++s)
                HIP_OK(hipMemcpyAsync(la.p + (size_t)s * N * dim, latents, (size_t)N * dim * sizeof(h16), hipMemcpyDeviceToDevice, st));
        for (const ResamplerLayer& L : layers) {
            const size_t mk = c.ar->mark();
            Act kvin = c.new_act(1, n * Nk, 1, dim);                            // per sample: LN1(x) rows, then LN2(lat) rows
            Act lnq = layer_norm(c, L.n2, la, eps);                             // LN2(lat) once, dense: to_q's operand ...
            if (!c.dry()) {
                // ... and its N rows per sample behind that sample's T rows of LN1(x): one strided copy of n x (N dim) halves
                HIP_OK(hipMemcpy2DAsync(kvin.p + (size_t)T * dim, (size_t)Nk * dim * sizeof(h16), lnq.p, (size_t)N * dim * sizeof(h16),
                                        (size_t)N * dim * sizeof(h16), (size_t)n, hipMemcpyDeviceToDevice, st));
                for (int s = 0; s < n; ++s)
                    c.check(ladi_launch_layernorm(xp.p + (size_t)s * T * dim, dim, L.n1.g, L.n1.b, eps, T, dim, kvin.p + (size_t)s * Nk * dim, dim, st),
                            "norm1");
            }
            Act kv = c.new_act(1, n * Nk, 1, 2 * inner), q = c.new_act(1, n * N, 1, inner), ao = c.new_act(1, n * N, 1, inner);
            linear(c, L.kv, kvin, kv, LADI_ACT_NONE, nullptr);
            linear(c, L.q, lnq, q, LADI_ACT_NONE, nullptr);
            if (!c.dry()) {
                AttnArgs aa;
                aa.q = q.p; aa.k = kv.p; aa.v = kv.p + inner; aa.o = ao.p;
                aa.ldq = inner; aa.ldk = aa.ldv = 2 * inner; aa.ldo = inner;
                aa.sq = (long long)N * inner; aa.sk = aa.sv = (long long)Nk * 2 * inner; aa.so = (long long)N * inner;
                aa.n = n; aa.heads = heads; aa.Nq = N; aa.Nk = Nk; aa.scale = 1.f / std::sqrt((float)dim_head); aa.causal = 0;
                if (dim_head == 64) c.check(ladi_launch_flash_attn64(aa, st), "resampler attention");
                else c.check(ladi_launch_attn_generic(aa, dim_head, st), "resampler attention");
            }
            linear(c, L.o, ao, lb, LADI_ACT_NONE, &la);                         // lb = to_out(a) + la
            Act f = layer_norm(c, L.ffn, lb, eps);
            Act m = c.new_act(1, n * N, 1, L.w1.cout);
            linear(c, L.w1, f, m, LADI_ACT_GELU, nullptr);
            linear(c, L.w2, m, la, LADI_ACT_NONE, &lb);                         // la = W2(gelu(W1(LN(lb)))) + lb
            c.ar->release(mk);
        }
        Act po = c.new_act(1, n * N, 1, out_dim);
        linear(c, proj_out, la, po, LADI_ACT_NONE, nullptr);
        if (!c.dry())
            c.check(ladi_launch_layernorm(po.p, out_dim, norm_out.g, norm_out.b, eps, n * N, out_dim, tokens_out, out_dim, st), "norm_out");
    });
}

}  // namespace ladi
