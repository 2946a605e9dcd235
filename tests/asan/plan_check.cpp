// CPU-only exercise of the host side of libcae_hip under AddressSanitizer: plan creation / tensor tables / error paths /
// destruction of the ConvAE engine (plain and trunk mode through the var engine), the UNET engine (with its kernel plan) and the
// Linear engine.
// No GPU call is made.
#include <cstdio>
#include <cstring>
#include <vector>
#include "cae_hip.h"
#include "cae_linear.h"
#include "cae_vae.h"
#include "cae_unet.h"

static std::vector<cae_layer_spec> enc_layers(int h, int n, int c0) {
    std::vector<cae_layer_spec> v;
    int c = c0, s = h;
    for (int i = 0; i < n; i++) {
        cae_layer_spec l{c, s, s, c * 2, (s - 3) / 2 + 1, (s - 3) / 2 + 1, 3, 3, 2, 0};
        v.push_back(l);
        c *= 2;
        s = (s - 3) / 2 + 1;
    }
    return v;
}
static std::vector<cae_layer_spec> dec_layers(int h, int n, int c0, int last_k) {
    std::vector<cae_layer_spec> v;
    int c = c0, s = h;
    for (int i = 0; i < n; i++) {
        const int k = i == n - 1 ? last_k : 3;
        const int co = c / 2 > 0 ? c / 2 : 1;
        cae_layer_spec l{c, s, s, co, (s - 1) * 2 + k, (s - 1) * 2 + k, k, k, 2, 0};
        v.push_back(l);
        c = co;
        s = (s - 1) * 2 + k;
    }
    return v;
}

// a UNET of k4 s2 p1 layers: encoder in_c -> channels[0] -> ..., decoder back up to out_c with the skip concat
static void unet_layers(int in_c, int out_c, int size, const std::vector<int>& ch, std::vector<cae_layer_spec>& enc,
                        std::vector<cae_layer_spec>& dec) {
    const int n = (int)ch.size();
    std::vector<int> c{in_c}, s{size};
    for (int i = 0; i < n; i++) {
        c.push_back(ch[i]);
        s.push_back(s.back() / 2);
        enc.push_back(cae_layer_spec{c[i], s[i], s[i], c[i + 1], s[i + 1], s[i + 1], 4, 4, 2, 1});
    }
    for (int j = 0; j < n; j++) {
        const int src = n - j, dst = n - j - 1;
        dec.push_back(cae_layer_spec{j == 0 ? c[src] : 2 * c[src], s[src], s[src], j < n - 1 ? c[dst] : out_c, s[dst], s[dst], 4, 4, 2, 1});
    }
}

// an all-reduce callback that sums nothing (the shard checks refuse before any table is passed)
static int no_allreduce(void*, void*, int64_t) { return 0; }

int main() {
    int failures = 0;
    auto expect = [&](bool ok, const char* what) {
        if (!ok) {
            printf("FAILED: %s (%s)\n", what, cae_last_error());
            failures++;
        }
    };
    for (int rep = 0; rep < 3; rep++) {
        auto enc = enc_layers(16, 2, 1);
        auto dec = dec_layers(3, 6, 64, 4);
        cae_engine* e = nullptr;
        expect(cae_engine_create(enc.data(), (int)enc.size(), dec.data(), (int)dec.size(), 128, 32, 64, &e) == 0, "cae_engine_create");
        if (e) {
            cae_tensor_info_t t;
            long long total = 0;
            for (int i = 0; i < cae_tensor_count(e); i++) {
                expect(cae_tensor_info(e, i, &t) == 0, "cae_tensor_info");
                if (t.arena == 0) total += t.numel;
            }
            expect(total == 112271, "parameter count of the benchmark geometry");
            expect(cae_tensor_info(e, cae_tensor_count(e), &t) != 0, "tensor index out of range is refused");
            expect(cae_workspace_bytes(e) > 0 && cae_param_count(e) >= total, "sizes");
            expect(cae_train_step(e, 0, nullptr, 64) != 0, "a step on an unbound engine is refused");
            expect(cae_set_cursor(e, 0, 0) != 0, "cursor on an unbound engine is refused");
            char plan[4096];
            expect(cae_debug_plan(e, 64, 1, plan, sizeof plan) == 0 && strstr(plan, "dec5 fwd=last_fused<2,1,4,4> hb=4 vec4=1 bn=1 bwd=(fused)"),
                   "cae_debug_plan");
            expect(cae_debug_plan(e, 64, 0, plan, sizeof plan) == 0 && strstr(plan, "tail bwd=-"), "cae_debug_plan (eval)");
            expect(cae_set_kernel_mode(e, 0) == 0 && cae_debug_plan(e, 8, 1, plan, sizeof plan) == 0 && strstr(plan, "dec5 fwd=up bwd=wgrad+down"),
                   "cae_debug_plan (generic kernels)");
            expect(cae_debug_plan(e, 65, 1, plan, sizeof plan) != 0, "a plan beyond max_batch is refused");
            expect(cae_debug_plan(e, 64, 1, plan, 16) != 0, "too small a plan buffer is refused");
            cae_engine_destroy(e);
        }
        // broken geometry: messages, no leak
        auto bad = dec;
        bad[2].out_h += 1;
        cae_engine* b = nullptr;
        expect(cae_engine_create(enc.data(), 2, bad.data(), 6, 128, 32, 64, &b) != 0 && b == nullptr, "inconsistent decoder is refused");
        expect(cae_engine_create(nullptr, 0, dec.data(), 6, 128, 32, 64, &b) != 0, "null encoder is refused");
        // the 'var' engine = a trunk-mode ConvAE engine inside
        auto venc = enc_layers(64, 4, 1);
        auto vdec = dec_layers(3, 7, 128, 4);
        vae_engine* v = nullptr;
        expect(vae_engine_create(venc.data(), 4, vdec.data(), 7, 128, 32, 16, &v) == 0, "vae_engine_create");
        if (v) {
            cae_tensor_info_t t;
            bool mu = false, lv = false;
            for (int i = 0; i < vae_tensor_count(v); i++) {
                expect(vae_tensor_info(v, i, &t) == 0, "vae_tensor_info");
                mu |= !strcmp(t.name, "enc/encoder_mu.weight");
                lv |= !strcmp(t.name, "enc/encoder_logvar.bias");
            }
            expect(mu && lv, "the heads are listed under the var model's names");
            expect(vae_train_step(v, 0, nullptr, 0, 16, 0) != 0, "a step on an unbound var engine is refused");
            char plan[4096];
            expect(vae_debug_plan(v, 16, 1, plan, sizeof plan) == 0 && strstr(plan, "head fwd=layers why=variational") &&
                       strstr(plan, "tail bwd=layers why=variational") && strstr(plan, "fc2 bwd=pair burst=1"),
                   "vae_debug_plan");
            expect(vae_debug_plan(v, 17, 1, plan, sizeof plan) != 0, "var: a plan beyond max_batch is refused");
            expect(vae_trunk_debug_read(v, "glast", 0, plan, 4) < 0, "var: a trunk read on an unbound engine is refused");
            float g[1];
            expect(vae_forward_backward_sync(v, 0, nullptr, 0, 3, 2, 4, 1, 0, g, no_allreduce, nullptr) == CAE_ERR_ARG,
                   "var: a shard past the global batch is refused");
            expect(vae_forward_backward_sync(v, 0, nullptr, 0, 2, 0, 4, 1, 0, g, nullptr, nullptr) == CAE_ERR_ARG,
                   "var: a shard without a callback is refused");
            vae_engine_destroy(v);
        }
        auto small = dec_layers(3, 5, 64, 4);   // 128x128 output: MS-SSIM needs >= 176
        expect(vae_engine_create(enc.data(), 2, small.data(), 5, 16, 4, 4, &v) != 0, "too small an output for MS-SSIM is refused");
        // the Linear engine: sizes, an unbound step, bad arguments
        lin_engine* l = nullptr;
        expect(lin_engine_create(8, 32, 5, &l) == 0, "lin_engine_create");
        if (l) {
            double loss[2];
            float dummy[4];
            expect(lin_param_count(l) == 32 * 8 + 32, "lin_param_count");
            expect(lin_workspace_bytes(l) > 0 && lin_loss_slots(l) == 4096, "Linear sizes");
            expect(lin_train_step(l, 0, nullptr, 0, 5, 0) != 0, "a step on an unbound Linear engine is refused");
            expect(lin_score(l, dummy, 1, dummy) != 0, "scoring on an unbound Linear engine is refused");
            expect(lin_read_losses(l, 4095, 2, loss) != 0, "loss slots out of range are refused");
            expect(lin_set_dataset(l, 2, dummy, dummy, 4) != 0 && lin_set_dataset(l, 0, nullptr, dummy, 4) != 0, "bad data sets are refused");
            expect(lin_set_step(l, -1) != 0, "a negative step is refused");
            expect(lin_bind(l, dummy, dummy, nullptr, dummy, 1 << 30) != 0, "a null arena is refused");
            lin_engine_destroy(l);
        }
        // a six-level UNET (64 px down to a 1x1 bottleneck): more repacked layers than one repack launch takes; its kernel plan
        std::vector<cae_layer_spec> uenc, udec;
        unet_layers(1, 1, 64, {8, 8, 16, 16, 16, 16}, uenc, udec);
        unet_engine* u = nullptr;
        expect(unet_engine_create(uenc.data(), 6, udec.data(), 6, 16, 4, 4, &u) == 0, "unet_engine_create (6 levels)");
        if (u) {
            char plan[4096];
            expect(unet_debug_plan(u, 4, 1, plan, sizeof plan) == 0 && strstr(plan, "pack entries=10 launches=2"), "unet_debug_plan");
            expect(unet_debug_plan(u, 4, 0, plan, sizeof plan) == 0 && strstr(plan, "dec5 "), "unet_debug_plan (eval)");
            expect(unet_debug_plan(u, 5, 1, plan, sizeof plan) != 0, "a plan beyond max_batch is refused");
            expect(unet_debug_plan(u, 4, 1, plan, 16) != 0, "too small a plan buffer is refused");
            expect(unet_train_step(u, 0, nullptr, 0, 4, 0) != 0, "a step on an unbound UNET engine is refused");
            float g[1];
            expect(unet_forward_backward_sync(u, 0, nullptr, 0, 3, 2, 4, 1, 0, g, no_allreduce, nullptr) == CAE_ERR_ARG,
                   "UNET: a shard past the global batch is refused");
            expect(unet_forward_backward_sync(u, 0, nullptr, 0, 2, 0, 4, 1, 0, g, nullptr, nullptr) == CAE_ERR_ARG,
                   "UNET: a shard without a callback is refused");
            unet_engine_destroy(u);
        }
        udec[5].out_c = 2;
        udec[4].out_c = 4;   // a skip concat that does not match
        expect(unet_engine_create(uenc.data(), 6, udec.data(), 6, 16, 4, 4, &u) != 0, "a broken UNET is refused");
        expect(lin_engine_create(0, 32, 5, &l) != 0 && lin_engine_create(1 << 20, 1 << 20, 5, &l) != 0, "bad Linear sizes are refused");
    }
    printf(failures ? "%d checks failed\n" : "host-side plan checks clean (%d)\n", failures);
    return failures ? 1 : 0;
}
