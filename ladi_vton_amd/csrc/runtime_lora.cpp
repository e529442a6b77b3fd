// LoRA adapters of the native UNet: the target table, adapter storage, the device-side merge (lora.hip) and the weight read-back.
// The merge keeps every weight at its address: captured graphs, lanes, tile selections and arenas stay valid and the forward launches what
// it launched before.  What a changed weight invalidates is dropped by lora_set: the cross-attention K/V cache (ctx_n = 0, so a stand-alone
// forward fails with the set_context error instead of using stale K/V), the stand-alone feature cache rows, and the re-packed operands of
// the fused sub-blocks (packed again from the merged o2 / ff2).
#include "runtime.h"
#include <algorithm>
#include <cmath>
#include <cstring>

namespace ladi {

#define HIP_OK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) throw std::runtime_error(std::string(#x) + ": " + hipGetErrorString(e_)); } while (0)

LoraAdapter::~LoraAdapter() { if (dev) (void)hipFree(dev); }

void UNet::build_lora_targets() {
    lora_targets.clear(); lora_index.clear();
    auto add = [&](const std::string& name, DConv& cv, int row0 = 0, int rows = -1, int geglu_half = 0, XfBlock* xf = nullptr, int packed = 0) {
        LoraTarget t; t.name = name; t.cv = &cv; t.row0 = row0; t.rows = rows < 0 ? cv.cout : rows; t.geglu_half = geglu_half; t.xf = xf; t.packed = packed;
        lora_index.emplace(name, (int)lora_targets.size());
        lora_targets.push_back(std::move(t));
    };
    auto add_res = [&](ResBlock& r, const std::string& p) {
        add(p + ".conv1", r.c1); add(p + ".conv2", r.c2);
        if (r.has_sc) add(p + ".conv_shortcut", r.sc);
        add(p + ".time_emb_proj", temb_all, r.temb_off, r.cout);
    };
    auto add_xf = [&](XfBlock& x) {
        const std::string& p = x.prefix;
        const std::string b = p + ".transformer_blocks.0";
        const int C = x.C;
        add(p + ".proj_in", x.proj_in);
        add(b + ".attn1.to_q", x.qkv, 0, C); add(b + ".attn1.to_k", x.qkv, C, C); add(b + ".attn1.to_v", x.qkv, 2 * C, C);
        add(b + ".attn1.to_out.0", x.o1);
        add(b + ".attn2.to_q", x.q2);
        add(b + ".attn2.to_k", x.kv2, 0, C); add(b + ".attn2.to_v", x.kv2, C, C);
        add(b + ".attn2.to_out.0", x.o2, 0, -1, 0, &x, 1);
        add(b + ".ff.net.0.proj", x.ff1, 0, -1, x.ff1.cout / 2);
        add(b + ".ff.net.2", x.ff2, 0, -1, 0, &x, 2);
        add(p + ".proj_out", x.proj_out);
    };
    const int L = cfg.layers_per_block;
    add("conv_in", conv_in);
    add("time_embedding.linear_1", time_l1); add("time_embedding.linear_2", time_l2);
    int ri = 0, xi = 0;
    for (int i = 0; i < 4; ++i) {
        const std::string p = "down_blocks." + std::to_string(i);
        for (int j = 0; j < L; ++j) {
            add_res(down_res[ri++], p + ".resnets." + std::to_string(j));
            if (i < 3) add_xf(xf[xi++]);
        }
        if (i < 3) add(p + ".downsamplers.0.conv", down_samp[i]);
    }
    add_res(mid_res[0], "mid_block.resnets.0");
    add_xf(xf[xi++]);
    add_res(mid_res[1], "mid_block.resnets.1");
    ri = 0;
    for (int i = 0; i < 4; ++i) {
        const std::string p = "up_blocks." + std::to_string(i);
        for (int j = 0; j < L + 1; ++j) {
            add_res(up_res[ri++], p + ".resnets." + std::to_string(j));
            if (i > 0) add_xf(xf[xi++]);
        }
        if (i < 3) add(p + ".upsamplers.0.conv", up_samp[i]);
    }
    add("conv_out", conv_out);
}

static bool ends_with(const std::string& s, const char* suf) {
    const size_t n = std::strlen(suf);
    return s.size() >= n && s.compare(s.size() - n, n, suf) == 0;
}

void UNet::lora_load(const std::string& name, const WeightStore& ws) {
    if (name.empty()) throw std::runtime_error("empty adapter name");
    for (auto& a : lora_adapters)
        if (a->name == name) throw std::runtime_error("an adapter named '" + name + "' is already loaded");
    if ((int)lora_adapters.size() >= LORA_MAX_ADAPTERS)
        throw std::runtime_error("at most " + std::to_string((int)LORA_MAX_ADAPTERS) + " adapters can be loaded (delete one first)");
    // ---- validate everything, lay the factors out; nothing of the UNet changes before the end of this block
    struct Item { int ti; int rank; float alpha; const HostTensor* up; const HostTensor* down; size_t off_up, off_down; };
    std::vector<Item> items;
    size_t floats = 0;
    static const char* const kDown = ".lora_down.weight"; static const char* const kUp = ".lora_up.weight"; static const char* const kAlpha = ".alpha";
    for (auto& kv : ws.m) {
        const std::string& k = kv.first;
        if (ends_with(k, kUp) || ends_with(k, kAlpha)) {
            const std::string mod = k.substr(0, k.size() - std::strlen(ends_with(k, kUp) ? kUp : kAlpha));
            if (!ws.has(mod + kDown)) throw std::runtime_error(k + ": no " + mod + kDown + " beside it");
            continue;
        }
        if (!ends_with(k, kDown)) throw std::runtime_error("unexpected key '" + k + "' (want <module>.lora_down.weight, .lora_up.weight, .alpha)");
        const std::string mod = k.substr(0, k.size() - std::strlen(kDown));
        auto it = lora_index.find(mod);
        if (it == lora_index.end()) throw std::runtime_error("unknown module '" + mod + "': not a conv / linear of this UNet");
        const LoraTarget& T = lora_targets[it->second];
        if (!ws.has(mod + kUp)) throw std::runtime_error(mod + ": lora_up.weight is missing");
        const HostTensor& dn = kv.second; const HostTensor& up = ws.get(mod + kUp);
        const int taps = T.cv->k * T.cv->k, cin = T.cv->cin;
        auto shape_str = [](const HostTensor& t) { std::string s = "["; for (size_t i = 0; i < t.shape.size(); ++i) s += (i ? ", " : "") + std::to_string(t.shape[i]); return s + "]"; };
        if (dn.shape.size() != 2 && dn.shape.size() != 4) throw std::runtime_error(mod + ": lora_down of shape " + shape_str(dn) + " is neither 2-D nor 4-D");
        const long long r = dn.shape[0];
        if (r < 1 || r > LORA_MAX_RANK) throw std::runtime_error(mod + ": rank " + std::to_string(r) + " outside [1, " + std::to_string((int)LORA_MAX_RANK) + "]");
        const long long dtaps = dn.shape.size() == 4 ? dn.shape[2] * dn.shape[3] : 1;
        if (dn.shape[1] != cin || dtaps != taps || (dn.shape.size() == 4 && dn.shape[2] != dn.shape[3]))
            throw std::runtime_error(mod + ": lora_down of shape " + shape_str(dn) + " does not fit the module (in " + std::to_string(cin) + ", kernel " +
                                     std::to_string(T.cv->k) + ")");
        bool up_ok = up.shape.size() >= 2 && up.shape[0] == T.rows && up.shape[1] == r;
        for (size_t i = 2; i < up.shape.size(); ++i) up_ok = up_ok && up.shape[i] == 1;
        if (!up_ok) throw std::runtime_error(mod + ": lora_up of shape " + shape_str(up) + " does not fit the module (out " + std::to_string(T.rows) +
                                             ", rank " + std::to_string(r) + ")");
        float alpha = (float)r;
        if (ws.has(mod + kAlpha)) {
            const HostTensor& al = ws.get(mod + kAlpha);
            if (al.numel() != 1 || !std::isfinite(al.data[0])) throw std::runtime_error(mod + ": alpha has to be one finite number");
            alpha = al.data[0];
        }
        Item it2{it->second, (int)r, alpha, &up, &dn, floats, 0};
        floats += ((size_t)T.rows * r + 3) & ~(size_t)3;
        it2.off_down = floats;
        floats += ((size_t)r * taps * cin + 3) & ~(size_t)3;
        items.push_back(it2);
    }
    if (items.empty()) throw std::runtime_error("the adapter holds no factor pair");
    // ---- stage on the host: up as it is, down tap-major [r][taps][cin] (diffusers: [r][cin][kh][kw])
    std::vector<float> host(floats, 0.f);
    for (auto& it : items) {
        const LoraTarget& T = lora_targets[it.ti];
        const int taps = T.cv->k * T.cv->k, cin = T.cv->cin;
        std::memcpy(&host[it.off_up], it.up->data.data(), (size_t)T.rows * it.rank * sizeof(float));
        for (int r = 0; r < it.rank; ++r)
            for (int i = 0; i < cin; ++i)
                for (int t = 0; t < taps; ++t)
                    host[it.off_down + ((size_t)r * taps + t) * cin + i] = it.down->data[((size_t)r * cin + i) * taps + t];
    }
    std::unique_ptr<LoraAdapter> ad(new LoraAdapter());
    ad->name = name;
    HIP_OK(hipMalloc(reinterpret_cast<void**>(&ad->dev), floats * sizeof(float)));
    HIP_OK(hipMemcpy(ad->dev, host.data(), floats * sizeof(float), hipMemcpyHostToDevice));
    for (auto& it : items) {
        LoraFactor f; f.rank = it.rank; f.alpha = it.alpha; f.up = ad->dev + it.off_up; f.down = ad->dev + it.off_down;
        ad->f.emplace(it.ti, f);
    }
    // ---- pristine copies of the packed weights this adapter is the first to touch (a weight no adapter has touched still holds its base)
    if (!lora_cnt) {
        lora_cnt = reinterpret_cast<unsigned*>(pool.alloc(lora_targets.size() * sizeof(unsigned)));
        HIP_OK(hipMemset(lora_cnt, 0, lora_targets.size() * sizeof(unsigned)));
    }
    for (auto& it : items) {
        const DConv& cv = *lora_targets[it.ti].cv;
        if (lora_base.count(cv.w)) continue;
        const size_t bytes = (size_t)cv.cout * cv.K() * sizeof(h16);
        h16* b = reinterpret_cast<h16*>(pool.alloc(bytes));
        HIP_OK(hipMemcpy(b, cv.w, bytes, hipMemcpyDeviceToDevice));
        lora_base.emplace(cv.w, b);
    }
    HIP_OK(hipDeviceSynchronize());
    lora_adapters.push_back(std::move(ad));
}

void UNet::lora_delete(const std::string& name) {
    for (auto& a : lora_active)
        if (a.first == name) throw std::runtime_error("adapter '" + name + "' is active (set_adapters without it first)");
    for (size_t i = 0; i < lora_adapters.size(); ++i)
        if (lora_adapters[i]->name == name) {
            HIP_OK(hipDeviceSynchronize());     // a merge that reads its factors may still be in flight
            lora_adapters.erase(lora_adapters.begin() + i);
            return;
        }
    throw std::runtime_error("no adapter named '" + name + "'");
}

namespace {
const LoraAdapter* find_adapter(const UNet& u, const std::string& name) {
    for (auto& a : u.lora_adapters)
        if (a->name == name) return a.get();
    return nullptr;
}
// re-merge the blocks `touched` from their base copies with the adapters of `set`; cnt: per-target non-finite counters or null
void merge_set(UNet& u, const std::vector<std::pair<std::string, float>>& set, const std::vector<char>& touched, unsigned* cnt, hipStream_t st) {
    for (size_t ti = 0; ti < u.lora_targets.size(); ++ti) {
        if (!touched[ti]) continue;
        const LoraTarget& T = u.lora_targets[ti];
        const DConv& cv = *T.cv;
        LoraMergeArgs a; std::memset(&a, 0, sizeof(a));
        a.base = u.lora_base.at(cv.w); a.W = cv.w; a.pitch = cv.K();
        a.cin = cv.cin; a.cin_pad = cv.cin_pad; a.taps = cv.k * cv.k;
        a.row0 = T.row0; a.rows = T.rows; a.geglu_half = T.geglu_half;
        for (auto& s : set) {
            const LoraAdapter* ad = find_adapter(u, s.first);
            auto f = ad->f.find((int)ti);
            if (f == ad->f.end()) continue;
            const int i = a.n_adapters++;
            a.up[i] = f->second.up; a.down[i] = f->second.down; a.rank[i] = f->second.rank;
            a.scale[i] = (float)((double)s.second * (double)f->second.alpha / (double)f->second.rank);
        }
        a.nonfinite = cnt ? cnt + ti : nullptr;
        const int rc = ladi_launch_lora_merge(a, st);
        if (rc) throw std::runtime_error("lora_merge of " + T.name + " refused or failed (rc = " + std::to_string(rc) + ")");
    }
    // the fused sub-blocks read o2 / ff2 re-packed
    for (size_t ti = 0; ti < u.lora_targets.size(); ++ti) {
        const LoraTarget& T = u.lora_targets[ti];
        if (!touched[ti] || !T.packed || !T.xf || !T.xf->o2_packed) continue;
        const int rc = T.packed == 1 ? ladi_launch_pack_wo(T.xf->o2.w, T.xf->o2_packed, st) : ladi_launch_pack_w2(T.xf->ff2.w, T.xf->ff2_packed, st);
        if (rc) throw std::runtime_error("re-packing the fused operand of " + T.name + " failed (rc = " + std::to_string(rc) + ")");
    }
}
}  // namespace

void UNet::lora_set(const std::vector<std::pair<std::string, float>>& set, hipStream_t st) {
    if ((int)set.size() > LORA_MAX_ADAPTERS) throw std::runtime_error("more than " + std::to_string((int)LORA_MAX_ADAPTERS) + " active adapters");
    for (size_t i = 0; i < set.size(); ++i) {
        if (!find_adapter(*this, set[i].first)) throw std::runtime_error("no adapter named '" + set[i].first + "'");
        if (!std::isfinite(set[i].second)) throw std::runtime_error("the weight of adapter '" + set[i].first + "' is not finite");
        for (size_t j = 0; j < i; ++j)
            if (set[j].first == set[i].first) throw std::runtime_error("adapter '" + set[i].first + "' is named twice");
    }
    std::vector<char> touched(lora_targets.size(), 0);
    bool any = false;
    const std::vector<std::pair<std::string, float>>* both[2] = {&set, &lora_active};
    for (auto* s : both)
        for (auto& e : *s)
            for (auto& f : find_adapter(*this, e.first)->f) { touched[f.first] = 1; any = true; }
    if (!any) { lora_active = set; return; }
    // the live weights are rewritten in place: nothing queued on ANY stream may still be reading them (a forward or a try-on run on another
    // stream), so the device is idle before the first merge
    HIP_OK(hipDeviceSynchronize());
    // what was computed from the old weights is dropped first: from here on no path can use it, whatever happens below
    ctx_n = 0;
    fc_rows.clear();
    // on any failure the previous set is merged back; if even that fails the error says that the weights are inconsistent
    auto merge_back = [&](const std::string& why) {
        try {
            merge_set(*this, lora_active, touched, nullptr, st);
            HIP_OK(hipStreamSynchronize(st));
        } catch (const std::exception& e) {
            throw std::runtime_error(why + "; merging the previous adapters back failed too (" + e.what() +
                                     "): the weights are INCONSISTENT, call set_adapters again or rebuild the UNet");
        }
        throw std::runtime_error(why + "; the previous adapters are back in place");
    };
    std::vector<unsigned> cnt(lora_targets.size());
    try {
        HIP_OK(hipMemsetAsync(lora_cnt, 0, lora_targets.size() * sizeof(unsigned), st));
        merge_set(*this, set, touched, lora_cnt, st);
        HIP_OK(hipMemcpyAsync(cnt.data(), lora_cnt, cnt.size() * sizeof(unsigned), hipMemcpyDeviceToHost, st));
        HIP_OK(hipStreamSynchronize(st));
    } catch (const std::exception& e) {
        merge_back(std::string("the merge failed (") + e.what() + ")");
    }
    for (size_t ti = 0; ti < cnt.size(); ++ti)
        if (cnt[ti])
            merge_back("the merged weight of " + lora_targets[ti].name + " has " + std::to_string(cnt[ti]) + " elements outside the fp16 range");
    lora_active = set;
}

long long UNet::export_weight(const std::string& key, float* host_out, long long cap) {
    static const char* const kW = ".weight";
    if (!ends_with(key, kW)) throw std::runtime_error("'" + key + "' is not a .weight key");
    auto it = lora_index.find(key.substr(0, key.size() - std::strlen(kW)));
    if (it == lora_index.end()) throw std::runtime_error("'" + key + "' is not the weight of a conv / linear of this UNet");
    const LoraTarget& T = lora_targets[it->second];
    const DConv& cv = *T.cv;
    const int taps = cv.k * cv.k, cin = cv.cin;
    const long long count = (long long)T.rows * cin * taps;
    if (!host_out) return count;
    if (cap < count) throw std::runtime_error(key + ": " + std::to_string(count) + " elements do not fit the buffer of " + std::to_string(cap));
    // the rows of the block in packed order (both row maps are permutations of [row0, row0 + rows)); the map is undone on the host
    std::vector<uint16_t> packed((size_t)T.rows * cv.K());
    HIP_OK(hipDeviceSynchronize());
    HIP_OK(hipMemcpy(packed.data(), cv.w + (size_t)T.row0 * cv.K(), packed.size() * sizeof(uint16_t), hipMemcpyDeviceToHost));
    for (int o = 0; o < T.rows; ++o) {
        int pr = o;
        if (T.geglu_half) { const int j = o < T.geglu_half ? o : o - T.geglu_half; pr = 64 * (j / 32) + j % 32 + (o < T.geglu_half ? 0 : 32); }
        const uint16_t* row = &packed[(size_t)pr * cv.K()];
        for (int t = 0; t < taps; ++t)
            for (int i = 0; i < cin; ++i) {
                _Float16 h; std::memcpy(&h, &row[(size_t)t * cv.cin_pad + i], 2);
                host_out[((size_t)o * cin + i) * taps + t] = (float)h;
            }
    }
    return count;
}

}  // namespace ladi
