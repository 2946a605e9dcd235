// engine_launch.h - host only: the launchers of the ConvAE step.  First the kernel families with template variants, in the
// order of their first use (template kernels are emitted in that order, and where code lands in engine.hip's code object has
// moved the step: DESIGN.md §4, "Code placement"), then one function per layer kind, which engine_step.h's loops call.
#pragma once

namespace {

// ---- specialised stride-2 kernels (kernels_s2.h): dispatch on (Cin, Cout, kh, kw) ----------------

// Launches a kernel of the k_s2_* families over tiles of tw x th covering an ex x ey extent of every image: sets the tile
// counts of its arguments; at most cap workgroups (they walk the remaining tiles).
template <class K, class A>
void s2_go(K kernel, A a, int ex, int ey, int tw, int th, int cap, hipStream_t s) {
    a.tiles_x = (ex + tw - 1) / tw;
    a.tiles_y = (ey + th - 1) / th;
    a.total_tiles = a.B * a.tiles_x * a.tiles_y;
    hipLaunchKernelGGL(kernel, dim3(a.total_tiles < cap ? a.total_tiles : cap), dim3(256), 0, s, a);
}

// false: this instantiation has no kernel for the pick (the chooser and the `if constexpr` guards below disagree)
template <int CIN, int COUT, int KH, int KW>
bool s2_fwd_launch(const S2Fwd& a, S2FwdPick p, hipStream_t s) {
    const int px = ((a.OW + 1) / 2 + 1) / 2, py = ((a.OH + 1) / 2 + 1) / 2;   // thread columns / rows per image (k_s2_fwd2)
    const int qx = (a.OW + 1) / 2, qy = (a.OH + 1) / 2;                       // quad columns / rows (k_s2_fwd, k_s2_fwd_cs)
    switch (p.k) {
        case S2F_CS:
            if constexpr (CIN * COUT * KH * KW > 80 && (256 / COUT) % 64 == 0) {
                constexpr int PIX = 256 / COUT;
                if (p.tw == 64) s2_go(k_s2_fwd_cs<CIN, COUT, KH, KW, 64>, a, qx, qy, 64, PIX / 64, kS2FwdCap, s);
                else s2_go(k_s2_fwd_cs<CIN, COUT, KH, KW, 32>, a, qx, qy, 32, PIX / 32, kS2FwdCap, s);
                return true;
            }
            return false;
        case S2F_QUAD:
            if (p.tw == 64) s2_go(k_s2_fwd<CIN, COUT, KH, KW, 64>, a, qx, qy, 64, 4, kS2FwdCap, s);
            else s2_go(k_s2_fwd<CIN, COUT, KH, KW, 32>, a, qx, qy, 32, 8, kS2FwdCap, s);
            return true;
        case S2F_WIDE:
            if (p.tw == 64) s2_go(k_s2_fwd2<CIN, COUT, KH, KW, 64>, a, px, py, 64, 4, kS2Fwd2Cap, s);
            else if (p.tw == 32) s2_go(k_s2_fwd2<CIN, COUT, KH, KW, 32>, a, px, py, 32, 8, kS2Fwd2Cap, s);
            else s2_go(k_s2_fwd2<CIN, COUT, KH, KW, 16>, a, px, py, 16, 16, kS2Fwd2Cap, s);
            return true;
    }
    return false;
}

// false: nothing launched (a shape outside S2_SHAPES x S2_KERNELS, or a pick the shape has no kernel for)
bool s2_fwd_dispatch(const ConvLayer& L, const S2Fwd& a, hipStream_t s) {
    const S2FwdPick p = choose_s2_fwd(L, a.B, a.epi);
    return s2_for_shape(L, [&](auto sh) { return s2_fwd_launch<sh.cin, sh.cout, sh.kh, sh.kw>(a, p, s); });
}

template <int CIN, int COUT, int KH, int KW>
bool s2_bwd_launch(const S2Bwd& a, S2BwdPick p, hipStream_t s) {   // false: as s2_fwd_launch
    switch (p.k) {
        case S2B_DIRECT:
            if constexpr (CIN * COUT * KH * KW <= 72) {
                if (p.tw == 64) s2_go(k_s2_bwd2<CIN, COUT, KH, KW, 64>, a, a.W, a.H, 64, 4, kS2BwdCap, s);
                else s2_go(k_s2_bwd2<CIN, COUT, KH, KW, 32>, a, a.W, a.H, 32, 8, kS2BwdCap, s);
                return true;
            }
            return false;
        case S2B_SPLIT:
            if constexpr (CIN * COUT * KH * KW > 72 && CIN == 8 && CIN * COUT * KH * KW / 4 <= 72) {
                // 2 channels per thread, 64 pixels (32 x 2) per workgroup pass
                s2_go(k_s2_bwd_split<CIN, 2, COUT, KH, KW, 32>, a, a.W, a.H, 32, 2, kS2BwdCap, s);
                return true;
            }
            return false;
        case S2B_GENERAL:
            if constexpr (CIN * COUT * KH * KW > 72 && !(CIN == 8 && CIN * COUT * KH * KW / 4 <= 72)) {
                constexpr int CT = (CIN % 2 == 0 && CIN != 6) ? 2 : 3;   // input channels per thread
                constexpr int CG = CIN / CT;                              // ci-groups per workgroup
                constexpr int PIX = 256 / CG;                             // pixels per tile
                constexpr int TPX = 32, TPY = PIX / 32;
                s2_go(k_s2_bwd<CIN, CT, COUT, KH, KW, TPX, TPY>, a, a.W, a.H, TPX, TPY, kS2BwdGeneralCap, s);
                return true;
            }
            return false;
    }
    return false;
}

bool s2_bwd_dispatch(const ConvLayer& L, const S2Bwd& a, hipStream_t s) {   // false: as s2_fwd_dispatch
    const S2BwdPick p = choose_s2_bwd(L);
    return s2_for_shape(L, [&](auto sh) { return s2_bwd_launch<sh.cin, sh.cout, sh.kh, sh.kw>(a, p, s); });
}

// ---- row-streaming kernels of the thin middle layers (kernels_rows.h): only where rows_bwd_ok holds ------------------------
template <int CIN, int CT, int COUT, int HB, int D>
void rows_go(S2Rows a, int lw, hipStream_t s) {
    constexpr int NB = 4 / (CIN / CT);
    const int hmax = a.H > a.QH - 1 ? a.H : a.QH - 1;
    a.bands = (hmax + HB - 1) / HB;
    const int imgs = 64 / lw;
    a.groups = (a.B + imgs - 1) / imgs;
    const dim3 grid((unsigned)(a.groups * ((a.bands + NB - 1) / NB)));
    if (imgs == 1) hipLaunchKernelGGL((k_s2_bwd_rows<CIN, CT, COUT, 3, 3, HB, 1, D>), grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL((k_s2_bwd_rows<CIN, CT, COUT, 3, 3, HB, 2, D>), grid, dim3(256), 0, s, a);
}

void rows_bwd_launch(const ConvLayer& L, S2Rows a, hipStream_t s) {
    const RowsPick p = choose_rows_bwd(L);
    a.QH = (L.hout + 1) / 2;
    if (L.cin == 4) rows_go<4, 4, 2, 2, 3>(a, p.lw, s);
    else rows_go<8, 2, 4, 4, 1>(a, p.lw, s);
}

template <int CIN, int COUT, int HB>
void rows_fwd_go(S2FwdRows a, int lw, hipStream_t s) {
    const int hmax = a.QH;
    a.bands = (hmax + HB - 1) / HB;
    const int imgs = 64 / lw;
    a.groups = (a.B + imgs - 1) / imgs;
    const dim3 grid((unsigned)(a.groups * ((a.bands + 3) / 4)));
    if (imgs == 1) hipLaunchKernelGGL((k_s2_fwd_rows<CIN, COUT, HB, 1>), grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL((k_s2_fwd_rows<CIN, COUT, HB, 2>), grid, dim3(256), 0, s, a);
}

void rows_fwd_launch(const ConvLayer& L, S2FwdRows a, hipStream_t s) {
    const RowsPick p = choose_rows_fwd(L);
    a.QH = (L.hout + 1) / 2;
    if (L.cin == 4) rows_fwd_go<4, 2, 2>(a, p.lw, s);
    else rows_fwd_go<8, 4, 1>(a, p.lw, s);
}

// ---- last decoder layer of a training step as one launch (kernels_last.h): forward + sigmoid + MSE + backward ---------
template <int CIN, int COUT, int KH, int KW>
bool last_fused_launch(S2Last a, LastPick p, int strips, hipStream_t s) {   // false: as s2_fwd_launch
    if constexpr (CIN * COUT * KH * KW <= 72) {
        a.QH = (a.OH + 1) / 2;
        a.QW = (a.OW + 1) / 2;
        const int hmax = a.H > a.QH - 1 ? a.H : a.QH - 1;
        a.strips = strips;
        a.bands = (hmax + kLastHB - 1) / kLastHB;
        a.total = a.B * a.strips * a.bands;
        const dim3 grid((a.total + 3) / 4);
        if (p.vec4 && p.bn) hipLaunchKernelGGL((k_s2_last_fused<CIN, COUT, KH, KW, kLastHB, true, true>), grid, dim3(256), 0, s, a);
        else if (p.bn) hipLaunchKernelGGL((k_s2_last_fused<CIN, COUT, KH, KW, kLastHB, false, true>), grid, dim3(256), 0, s, a);
        else hipLaunchKernelGGL((k_s2_last_fused<CIN, COUT, KH, KW, kLastHB, false, false>), grid, dim3(256), 0, s, a);
        return true;
    }
    return false;
}

bool last_fused_dispatch(const ConvLayer& L, const S2Last& a, hipStream_t s) {   // false: as s2_fwd_dispatch
    const LastPick p = choose_last(L, a.bn_in.mode != BN_NONE);
    return s2_for_shape(L, [&](auto sh) { return last_fused_launch<sh.cin, sh.cout, sh.kh, sh.kw>(a, p, last_strips(L), s); });
}

template <class K>
void head_lds_attr(K kernel, size_t bytes) {
    static size_t granted = 64 * 1024;
    if (bytes > granted) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
        granted = bytes;
    }
}

// ---- LDS-staged implicit-GEMM forward of a channel-rich stride-2 ConvTranspose2d (kernels_ctlds.h): where ct_fwd_plan holds
template <int KH, int KW>
void ct_fwd_go(const CtFwd& c, dim3 grid, int threads, size_t lds, hipStream_t s) {
    head_lds_attr(k_ct_fwd_lds<KH, KW>, lds);
    hipLaunchKernelGGL((k_ct_fwd_lds<KH, KW>), grid, dim3(threads), lds, s, c);
}

// ---- one function per layer kind ------------------------------------------------------------------------------------------
// Each builds its kernel's arguments from the operands its caller (engine_step.h) prepared once per layer, brackets the launch
// for the profile and launches; what every kind does after its launch (a SyncBN step's table exchange) is the caller's.

// encoder conv l (encoder.py:40-46): k_down, the producer's BatchNorm + ReLU in its prologue, BatchNorm sums in its epilogue
void enc_conv_fwd(cae_engine* e, const StepArgs& a, int l) {
    const ConvLayer& L = e->enc[l];
    Src big;
    BnDesc bnb = bn_none();
    if (l == 0) {
        big = src_plain(a.x_direct ? a.x_direct : e->ds_x[a.which], L.cin, L.hin, L.win);
        big.perm = a.x_direct ? nullptr : a.perm; big.use_cursor = a.x_direct ? 0 : 1; big.bump_adam = a.train ? 1 : 0;
    } else {
        const ConvLayer& P = e->enc[l - 1];
        big = src_plain(e->fptr(P.act_off), L.cin, L.hin, L.win);
        bnb = bn_of(e, P, a.train ? BN_BATCH : BN_RUNNING, (double)a.bn_batch * P.hout * P.wout, 1);
    }
    dim3 grid(grid1((int64_t)a.batch * L.hout * L.wout), L.cout);
    ProfScope _p(e, a.train ? "enc_conv_fwd" : "enc_conv_eval", l, bytes_fwd(a.batch, L));
    hipLaunchKernelGGL(k_down, grid, dim3(256), lds_bytes(L.cin, L.cout), e->stream, conv_geom(a.batch, L), big, bnb, e->params + L.w_off,
                       e->params + L.b_off, epi_raw_stats(e, L, a.train), bn_none(), (const StepState*)e->state());
}

// Linear i (encoder.py:54-58, decoder.py:31-35) of `in`; Linear 0 reads the last encoder layer P through its BatchNorm bn_p
void linear_fwd(cae_engine* e, const StepArgs& a, int i, const float* in, const ConvLayer& P, const BnDesc& bn_p) {
    const FcLayer& F = e->fc[i];
    const int B = a.batch, hw = P.hout * P.wout;
    ProfScope _p(e, e->use_s2 ? "linear_fwd_mfma" : "linear_fwd", i, bytes_lin_fwd(B, F));
    if (e->use_s2) {
        GemmArgs ga = zeroed<GemmArgs>();
        ga.M = B; ga.N = F.nout; ga.K = F.nin;
        ga.A = in; ga.sa_m = F.nin; ga.sa_k = 1;
        ga.B = e->params + F.w_off; ga.sb_k = 1; ga.sb_n = F.nin;   // B[k][n] = W[n][k]
        ga.C = e->fptr(F.act_off); ga.sc_m = F.nout; ga.sc_n = 1;
        ga.epi = GE_STORE; ga.bias = e->params + F.b_off; ga.relu = F.relu ? 1 : 0;
        ga.bn_a = i == 0 ? bn_p : bn_none(); ga.hw_a = hw; ga.bn_c = bn_none();
        const int tiles = ((B + 15) / 16) * ((F.nout + 15) / 16);
        hipLaunchKernelGGL(k_gemm16, dim3(tiles), dim3(256), gemm_lds(i == 0 ? P.cout : 0), e->stream, ga);
    } else {
        hipLaunchKernelGGL(k_lin_fwd, dim3(grid1((int64_t)B * F.nout)), dim3(256), lds_bytes(i == 0 ? P.cout : 0, 0),
                           e->stream, B, F.nin, F.nout, in, i == 0 ? bn_p : bn_none(), hw, e->params + F.w_off,
                           e->params + F.b_off, F.relu ? 1 : 0, e->fptr(F.act_off));
    }
}

// ---- forward: decoder conv-transposes (decoder.py:40-48) + sigmoid (:77) + MSELoss (conv_ae_model.py:303) -----------------

// What every forward family of decoder layer l reads and writes: its input with the producer's BatchNorm, and its epilogue in
// the shape-generic form (a middle layer: raw output + BatchNorm sums; the last: sigmoid and loss, or the raw output for a
// loss outside the trunk), which the specialised families take their operands from.
struct DecFwd { const ConvLayer& L; int l; bool last; Src in; BnDesc bn_in; Epi ep; };

DecFwd dec_fwd_operands(cae_engine* e, const StepArgs& a, int l) {
    const ConvLayer& L = e->dec[l];
    DecFwd c{L, l, l + 1 == (int)e->dec.size(), src_plain(e->fptr(l == 0 ? e->fc[3].act_off : e->dec[l - 1].act_off), L.cin, L.hin, L.win),
             bn_none(), {}};
    if (l > 0) c.bn_in = bn_of(e, e->dec[l - 1], a.train ? BN_BATCH : BN_RUNNING, (double)a.bn_batch * e->dec[l - 1].hout * e->dec[l - 1].wout, 1);
    Epi& ep = c.ep;
    if (c.last && a.external_loss) {   // raw output for a loss computed outside the trunk: no sigmoid, no statistics
        ep = epi_plain(e->fptr(e->off_zlast));
    } else if (!c.last) {
        ep = epi_raw_stats(e, L, a.train);
    } else {
        memset(&ep, 0, sizeof ep);
        // mean over the GLOBAL batch: each rank contributes sum(local terms) / global count, and the SUM all-reduce of the
        // gradients then yields the global-mean gradient (global_batch == batch on a single device)
        ep.inv_count = (float)(1.0 / ((double)a.global_batch * L.cout * L.hout * L.wout));
        ep.losses = e->losses(); ep.perm = a.perm; ep.use_cursor = a.use_cursor ? 1 : 0;
        ep.kind = a.train ? EPI_SIGMSE : EPI_SIGOUT;
        ep.target = a.train || a.want_loss ? e->ds_t[a.which] : nullptr;
        if (a.train) {
            ep.out = e->fptr(e->off_glast); ep.bias_acc = e->gradacc() + L.b_off;
        } else {
            ep.yhat = a.yhat;
        }
    }
    return c;
}

void fwd_rows(cae_engine* e, const StepArgs& a, const DecFwd& c) {
    const ConvLayer& L = c.L;
    S2FwdRows f = zeroed<S2FwdRows>();
    f.B = a.batch; f.H = L.hin; f.W = L.win; f.OH = L.hout; f.OW = L.wout;
    f.in = c.in.p; f.bn_in = c.bn_in;
    f.w = e->params + L.w_off; f.bias = e->params + L.b_off;
    f.out = c.ep.out; f.stats = a.train ? c.ep.stats : nullptr;
    ProfScope _p(e, a.train ? "s2_convt_fwd" : "s2_convt_eval", c.l, bytes_fwd(a.batch, L));
    rows_fwd_launch(L, f, e->stream);
}

int fwd_s2(cae_engine* e, const StepArgs& a, const DecFwd& c) {
    const ConvLayer& L = c.L;
    const Epi& ep = c.ep;
    S2Fwd f = zeroed<S2Fwd>();
    f.B = a.batch; f.H = L.hin; f.W = L.win; f.OH = L.hout; f.OW = L.wout;
    f.in = c.in.p; f.bn_in = c.bn_in;
    f.w = e->params + L.w_off; f.bias = e->params + L.b_off;
    f.st = e->state();
    f.epi = s2_fwd_epi(e, c.l, a.train, a.external_loss);
    f.out = f.epi == S2_SIGOUT ? ep.yhat : ep.out;
    if (!c.last) f.stats = ep.stats;
    if (f.epi == S2_SIGMSE || f.epi == S2_SIGOUT) {
        f.target = ep.target; f.perm = ep.perm; f.use_cursor = ep.use_cursor;
        f.losses = ep.losses; f.inv_count = ep.inv_count;
        f.bias_acc = e->sgacc() + L.sh_b; f.bias_stride = e->segs.n;
    }
    ProfScope _p(e, c.last ? (a.train ? "s2_convt_last_fwd_loss" : "s2_convt_last_eval") : (a.train ? "s2_convt_fwd" : "s2_convt_eval"), c.l,
                 bytes_fwd(a.batch, L, c.last && (a.train || a.want_loss)));
    return s2_fwd_dispatch(L, f, e->stream) ? CAE_OK : fail(CAE_ERR_STATE, "decoder layer %d: no k_s2_fwd kernel for the chosen variant", c.l);
}

// the layer's forward on k_ct_fwd_lds: only where ct_fwd_plan holds (choose_dec_fwd)
void fwd_ct_lds(cae_engine* e, const StepArgs& a, const DecFwd& c) {
    const ConvLayer& L = c.L;
    CtFwd f;
    int waves = 0; size_t lds = 0;
    (void)ct_fwd_plan(e, a.batch, L, c.l, f, waves, lds);
    f.in = c.in.p; f.bn_in = c.bn_in; f.w = e->params + L.w_off; f.bias = e->params + L.b_off;
    f.out = c.ep.out; f.stats = a.train ? c.ep.stats : nullptr;
    dim3 grid((unsigned)(a.batch * f.tg), (unsigned)((L.cout + 15) / 16));
    ProfScope _p(e, a.train ? "ct_convt_fwd" : "ct_convt_eval", c.l, bytes_fwd(a.batch, L));
    if (L.kh == 3 && L.kw == 3) ct_fwd_go<3, 3>(f, grid, 64 * waves, lds, e->stream);
    else if (L.kh == 4 && L.kw == 4) ct_fwd_go<4, 4>(f, grid, 64 * waves, lds, e->stream);
    else if (L.kh == 3 && L.kw == 4) ct_fwd_go<3, 4>(f, grid, 64 * waves, lds, e->stream);
    else ct_fwd_go<4, 3>(f, grid, 64 * waves, lds, e->stream);
}

void fwd_ig(cae_engine* e, const StepArgs& a, const DecFwd& c) {
    const ConvLayer& L = c.L;
    const IgFwdPlan p = ig_fwd_plan(L, a.batch);
    IgFwd f = zeroed<IgFwd>();
    f.B = a.batch; f.Cin = L.cin; f.H = L.hin; f.W = L.win; f.Cout = L.cout; f.OH = L.hout; f.OW = L.wout;
    f.KH = L.kh; f.KW = L.kw; f.QH = (L.hout + 1) / 2; f.QW = (L.wout + 1) / 2;
    f.in = c.in.p; f.bn_in = c.bn_in; f.w = e->params + L.w_off; f.bias = e->params + L.b_off;
    f.out = c.ep.out; f.stats = a.train ? c.ep.stats : nullptr;
    f.ksplit = p.ksplit; f.tiles_per_wave = p.tiles_per_wave;
    ProfScope _p(e, a.train ? "ig_convt_fwd" : "ig_convt_eval", c.l, bytes_fwd(a.batch, L));
    hipLaunchKernelGGL(k_ig_fwd_s2, p.grid, dim3(256), p.lds, e->stream, f);
}

void fwd_generic(cae_engine* e, const StepArgs& a, const DecFwd& c) {
    const ConvLayer& L = c.L;
    dim3 grid(grid1((int64_t)a.batch * L.hout * L.wout), L.cout);
    ProfScope _p(e, c.last ? (a.train ? "dec_convt_last_fwd_loss" : "dec_convt_last_eval") : (a.train ? "dec_convt_fwd" : "dec_convt_eval"), c.l,
                 bytes_fwd(a.batch, L, c.last && (a.train || a.want_loss)));
    hipLaunchKernelGGL(k_up, grid, dim3(256), lds_bytes(L.cin, L.cout), e->stream, conv_geom(a.batch, L), c.in, c.bn_in, e->params + L.w_off,
                       e->params + L.b_off, c.ep, bn_none(), (const StepState*)e->state());
}

// ---- backward: decoder conv-transposes -------------------------------------------------------------------------------------------

// What every backward kind of conv layer l (decoder or encoder) reads: the gradient wrt its raw output, masked by its own
// BatchNorm + ReLU (the last decoder layer's comes from the loss), its input activation, read through the producer's BatchNorm
// (the head of the encoder reads the data set), and its producer (where the input gradient goes).
struct ConvBwd { const ConvLayer& L; int l; bool last; Src gy; BnDesc bng; Src ain; Producer prod; };

ConvBwd conv_bwd_operands(cae_engine* e, const StepArgs& a, const std::vector<ConvLayer>& chain, int l) {
    const ConvLayer& L = chain[l];
    const bool dec = L.transposed, last = dec && l + 1 == (int)chain.size();
    ConvBwd c{L, l, last, src_plain(e->fptr(last ? e->off_glast : L.grad_off), L.cout, L.hout, L.wout), bn_none(), {},
              dec ? dec_producer(e, l) : enc_producer(e, l)};
    if (!last) {
        c.gy.q = e->fptr(L.act_off);
        c.bng = bn_of(e, L, BN_BWD, (double)a.bn_batch * L.hout * L.wout, 0);
    }
    c.ain = src_plain(l > 0 ? c.prod.yprev : (dec ? e->fptr(e->fc[3].act_off) : (a.x_direct ? a.x_direct : e->ds_x[a.which])), L.cin, L.hin, L.win);
    if (!dec && l == 0 && !a.x_direct) {
        c.ain.perm = a.perm;
        c.ain.use_cursor = 1;
    }
    return c;
}

int bwd_last_fused(cae_engine* e, const StepArgs& a, const ConvBwd& c) {
    const ConvLayer& L = c.L;
    S2Last f = zeroed<S2Last>();
    f.B = a.batch; f.H = L.hin; f.W = L.win; f.OH = L.hout; f.OW = L.wout;
    f.in = c.ain.p; f.w = e->params + L.w_off; f.bias = e->params + L.b_off;
    f.target = e->ds_t[a.which]; f.perm = a.perm; f.use_cursor = a.use_cursor ? 1 : 0;
    f.st = e->state(); f.losses = e->losses();
    // mean over the GLOBAL batch (see dec_fwd_operands)
    f.inv_count = (float)(1.0 / ((double)a.global_batch * L.cout * L.hout * L.wout));
    f.bias_acc = e->sgacc() + L.sh_b; f.wacc = e->sgacc() + L.sh_w; f.acc_stride = e->segs.n;
    // this launch is also the forward consumer of the producer's BatchNorm: batch statistics, saved for the layers behind
    f.bn_in = c.prod.P ? bn_of(e, *c.prod.P, BN_BATCH, (double)a.bn_batch * c.prod.P->hout * c.prod.P->wout, 1) : bn_none();
    f.gin = c.prod.gin; f.stats_in = c.prod.stats_in;
    ProfScope _p(e, "s2_convt_last_fused", c.l, bytes_bwd(a.batch, L, true, false));
    return last_fused_dispatch(L, f, e->stream) ? CAE_OK : fail(CAE_ERR_STATE, "decoder layer %d: no k_s2_last_fused kernel for the chosen variant", c.l);
}

void bwd_rows(cae_engine* e, const StepArgs& a, const ConvBwd& c) {
    const ConvLayer& L = c.L;
    S2Rows f = zeroed<S2Rows>();
    f.B = a.batch; f.H = L.hin; f.W = L.win; f.OH = L.hout; f.OW = L.wout;
    f.g = c.gy.p; f.yout = c.gy.q; f.bn_out = c.bng;
    f.ain = c.ain.p; f.bn_in = c.prod.bn_prev;
    f.w = e->params + L.w_off; f.wacc = e->sgacc() + L.sh_w; f.wacc_stride = e->segs.n;
    f.gin = c.prod.gin; f.stats_in = c.prod.stats_in;
    f.bg = bn_grad_out(e, L, a);
    const WSlab sl = wgrad_slab_of(e, a.batch, a.external_loss, c.l);
    if (sl.nparts) f.wslab = reinterpret_cast<double*>(e->ws + e->off_wslab + sl.off);
    ProfScope _p(e, "s2_convt_bwd", c.l, bytes_bwd(a.batch, L, false, false));
    rows_bwd_launch(L, f, e->stream);
}

int bwd_s2(cae_engine* e, const StepArgs& a, const ConvBwd& c) {
    const ConvLayer& L = c.L;
    S2Bwd f = zeroed<S2Bwd>();
    f.B = a.batch; f.H = L.hin; f.W = L.win; f.OH = L.hout; f.OW = L.wout;
    f.g = c.gy.p; f.yout = c.gy.q; f.bn_out = c.bng;
    f.ain = c.ain.p; f.bn_in = c.prod.bn_prev;
    f.w = e->params + L.w_off; f.wacc = e->sgacc() + L.sh_w; f.wacc_stride = e->segs.n;
    f.gin = c.prod.gin; f.stats_in = c.prod.stats_in;
    f.bg = bn_grad_out(e, L, a);
    // (this family's count takes the input twice at the head of the chain too: DESIGN.md §8)
    ProfScope _p(e, "s2_convt_bwd", c.l, bytes_bwd(a.batch, L, c.last, false));
    return s2_bwd_dispatch(L, f, e->stream) ? CAE_OK : fail(CAE_ERR_STATE, "decoder layer %d: no k_s2_bwd kernel for the chosen variant", c.l);
}

int bwd_ct_lds(cae_engine* e, const StepArgs& a, const ConvBwd& c) {
    const ConvLayer& L = c.L;
    CtBwdPlan cp;
    (void)ct_bwd_plan(e, a.batch, L, c.l, cp);
    CtBwd f = zeroed<CtBwd>();
    f.B = a.batch; f.Cin = L.cin; f.H = L.hin; f.W = L.win; f.Cout = L.cout; f.OH = L.hout; f.OW = L.wout;
    f.imgs = cp.imgs; f.wstr = cp.wstr; f.bands = cp.bands; f.hb = cp.hb;
    f.g = c.gy.p; f.yout = c.gy.q; f.bn_out = c.bng;
    f.ain = c.ain.p; f.bn_in = c.prod.bn_prev;
    f.w = e->params + L.w_off;
    f.wacc = L.sh_w >= 0 ? e->sgacc() + L.sh_w : e->gradacc() + L.w_off;
    f.wacc_stride = L.sh_w >= 0 ? e->segs.n : 0;
    f.gin = c.prod.gin; f.stats_prev = c.prod.stats_in;
    f.bg = bn_grad_out(e, L, a);
    const WSlab sl = wgrad_slab_of(e, a.batch, a.external_loss, c.l);
    if (sl.nparts) {
        // partial tiles stored; Linear 3's backward launch adds them up into the plain accumulator (the shards stay zero)
        f.wslab = reinterpret_cast<float*>(e->ws + e->off_wslab + sl.off);
        f.slab_kfull = sl.kfull; f.slab_ppg = sl.ppg;
    }
    ProfScope _p(e, "ct_convt_bwd", c.l, bytes_bwd(a.batch, L, c.last, c.l == 0));
    if (cae_internal::ctbwd_launch(&f, sizeof f, (unsigned)cp.groups, (unsigned)(L.cin / 16), (unsigned)cp.parts, cp.lds_launch, e->stream))
        return fail(CAE_ERR_ARG, "k_ct_bwd_lds: argument layout mismatch");
    return CAE_OK;
}

void bwd_ig(cae_engine* e, const StepArgs& a, const ConvBwd& c) {
    const ConvLayer& L = c.L;
    const int B = a.batch;
    const IgBwdPlan p = ig_bwd_plan(L, B);
    IgWgrad fw = zeroed<IgWgrad>();
    fw.B = B; fw.Cin = L.cin; fw.H = L.hin; fw.W = L.win; fw.Cout = L.cout; fw.OH = L.hout; fw.OW = L.wout;
    fw.KH = L.kh; fw.KW = L.kw; fw.S = L.stride;
    fw.ain = c.ain.p; fw.bn_in = c.prod.bn_prev; fw.g = c.gy.p; fw.yout = c.gy.q; fw.bn_out = c.bng;
    fw.wacc = e->gradacc() + L.w_off;
    fw.bg = bn_grad_out(e, L, a);
    fw.ksteps_per_block = p.per;
    IgDgrad fd = zeroed<IgDgrad>();
    fd.B = B; fd.Cin = L.cin; fd.H = L.hin; fd.W = L.win; fd.Cout = L.cout; fd.OH = L.hout; fd.OW = L.wout;
    fd.KH = L.kh; fd.KW = L.kw; fd.S = L.stride;
    fd.g = c.gy.p; fd.yout = c.gy.q; fd.bn_out = c.bng; fd.w = e->params + L.w_off;
    fd.gin = c.prod.gin; fd.yprev = c.prod.yprev; fd.bn_prev = c.prod.bn_prev; fd.stats_prev = c.prod.stats_in;
    fd.ksplit = p.ksplit; fd.tiles_per_wave = p.tiles_per_wave;
    ProfScope _p(e, "ig_convt_bwd_pair", c.l, bytes_bwd(B, L, c.last, c.l == 0));
    hipLaunchKernelGGL(k_ig_bwd_pair, dim3(p.grid), dim3(256), p.lds, e->stream, fw, fd, p.wtiles, p.chunks, p.w_n8, p.d_gx, p.d_gy,
                       p.d_group);
}

// shape-generic: k_wgrad (+ BatchNorm parameter gradients of this layer), then the input gradient on k_down
void bwd_generic(cae_engine* e, const StepArgs& a, const ConvBwd& c) {
    const ConvLayer& L = c.L;
    const int B = a.batch;
    const StepState* st = e->state();
    const ConvGeom g = conv_geom(B, L);
    {
        const int64_t nw = (int64_t)L.cin * L.cout * L.kh * L.kw;
        const int64_t pos = (int64_t)B * L.hin * L.win;
        const int ppb = wgrad_ppb(pos, nw);
        dim3 grid((unsigned)nw, (unsigned)((pos + ppb - 1) / ppb));
        ProfScope _p(e, "dec_convt_wgrad", c.l, bytes_bwd(B, L, c.last, true));
        hipLaunchKernelGGL(k_wgrad, grid, dim3(256), lds_bytes(L.cin, L.cout), e->stream, g, c.ain, c.prod.bn_prev, c.gy, c.bng,
                           e->gradacc() + L.w_off, ppb, bn_grad_out(e, L, a), st);
    }
    dim3 grid(grid1((int64_t)B * L.hin * L.win), L.cin);
    ProfScope _p(e, "dec_convt_dgrad", c.l, bytes_bwd(B, L, c.last, c.l == 0));
    hipLaunchKernelGGL(k_down, grid, dim3(256), lds_bytes(L.cout, L.cin), e->stream, g, c.gy, c.bng, e->params + L.w_off,
                       (const float*)nullptr, epi_gin(c.prod), c.prod.bn_prev, st);
}

// ---- backward: the Linear chain -----------------------------------------------------------------------------------------------
// grad_off of fc[i] holds dL/d(pre-activation of fc[i] output); P: the last encoder layer, whose BatchNorm'd output Linear 0 reads

// Linear 2..0 in one launch (tail_plan)
void tail_bwd(cae_engine* e, const StepArgs& a, const TailArgs& tail, size_t tail_lds) {
    double bytes = 0;
    for (int j = 0; j < 3; j++) bytes += bytes_lin_bwd_pair(a.batch, e->fc[j]);
    head_lds_attr(k_tail_bwd, tail_lds);
    ProfScope _p(e, "tail_bwd", 0, bytes);
    hipLaunchKernelGGL(k_tail_bwd, dim3((a.batch + 15) / 16, 4), dim3(kHeadThreads), tail_lds, e->stream, tail);
}

// the input of Linear i: the last encoder layer's output, the previous Linear's, or (trunk mode) the reparameterised z
const float* linear_in(const cae_engine* e, int i, const ConvLayer& P) {
    return e->fptr(i == 0 ? P.act_off : (i == 2 && e->variational ? e->off_vz : e->fc[i - 1].act_off));
}

// weight gradient and input gradient of Linear i as one launch of two GEMMs (k_gemm16_pair)
int linear_bwd_pair(cae_engine* e, const StepArgs& a, int i, const ConvLayer& P) {
    const FcLayer& F = e->fc[i];
    const int B = a.batch, hw = P.hout * P.wout;
    const float* gout = e->fptr(F.grad_off);
    const float* in = linear_in(e, i, P);
    BnDesc bni = i == 0 ? bn_of(e, P, BN_SAVED, 0, 0) : bn_none();
    double* acc = e->gradacc();
    // weight gradient: dW[o][i] = sum_b gout[b][o] * in[b][i], db[o] = sum_b gout[b][o] (ones column)
    GemmArgs gw = zeroed<GemmArgs>();
    gw.M = F.nout; gw.N = F.nin + 1; gw.K = B;
    gw.A = gout; gw.sa_m = 1; gw.sa_k = F.nout;       // A[m=o][k=b] = gout[b][o]
    gw.B = in; gw.sb_k = F.nin; gw.sb_n = 1;          // B[k=b][n=i] = in[b][i]
    gw.epi = GE_ACC64;
    gw.accW = acc + F.w_off; gw.accB = acc + F.b_off; gw.ones_col = 1;
    // input gradient: gin[b][i] = mask( sum_o gout[b][o] * W[o][i] )
    GemmArgs gd = zeroed<GemmArgs>();
    gd.M = B; gd.N = F.nin; gd.K = F.nout;
    gd.A = gout; gd.sa_m = F.nout; gd.sa_k = 1;
    gd.B = e->params + F.w_off; gd.sb_k = F.nin; gd.sb_n = 1;   // B[k=o][n=i] = W[o][i]
    gd.sc_m = F.nin; gd.sc_n = 1;
    size_t lds = gemm_lds(0);
    if (i == 2 && e->variational) {
        gd.C = e->fptr(e->off_vgz);   // dL/dz; the hook below turns it into the heads' gradient
        gd.epi = GE_STORE;
    } else if (i > 0) {
        const FcLayer& G = e->fc[i - 1];
        gd.C = e->fptr(G.grad_off); gd.H = e->fptr(G.act_off);
        gd.epi = G.relu ? GE_RELU_MASK : GE_STORE;
    } else {
        gd.C = e->fptr(P.grad_off); gd.H = e->fptr(P.act_off);
        gd.epi = GE_BN_MASK; gd.bn_c = bni; gd.hw_c = hw; gd.stats_c = e->bn_stats(P.bn_index);
        lds = gemm_lds(P.cout);
    }
    const int tiles_d = ((gd.M + 15) / 16) * ((gd.N + 15) / 16);
    if (i == 0) {
        // the first encoder Linear's input carries BatchNorm+ReLU: compute dW^T = act(in)^T * gout so
        // the transform sits on the A operand (channel = row / hw), store transposed; the ones ROW
        // of A yields the bias gradient
        gw.M = F.nin + 1; gw.N = F.nout; gw.K = B;
        gw.A = in; gw.sa_m = 1; gw.sa_k = F.nin;            // A[m=i][k=b] = in[b][i]
        gw.B = gout; gw.sb_k = F.nout; gw.sb_n = 1;         // B[k=b][n=o] = gout[b][o]
        gw.epi = GE_ACC64_T; gw.ones_col = 0; gw.ones_row = 1;
        gw.bn_a = bni; gw.hw_a = hw; gw.bn_a_by_row = 1;
    }
    {
        const int tiles_w = ((gw.M + 15) / 16) * ((gw.N + 15) / 16);
        ProfScope _p(e, "linear_bwd_pair_mfma", i, bytes_lin_bwd_pair(B, F));
        // the input gradient's contraction runs over nout: long for the last decoder Linear (576 at cfg2): burst variant
        // (gd as built above: unit strides along k in A and along n in B, A rows K floats apart, no BatchNorm mask but for i = 0)
        const bool burst = linear_bwd_burst(e, i);
        if (burst && gemm16_burst_lds(gd.K) > lds) lds = gemm16_burst_lds(gd.K);
        // Linear 3's launch, the first behind the decoder's backward, also folds the weight-gradient slabs that wrote (the
        // fold workgroups come first in the grid; the algorithmic bytes above stay the two GEMMs')
        const WFold fold = i == 3 ? wgrad_fold_of(e, wgrad_slab_table(e, B, a.external_loss, e->wslab_bytes)) : zeroed<WFold>();
        hipLaunchKernelGGL(k_gemm16_pair, dim3(fold.nwg + tiles_w + tiles_d), dim3(256), lds, e->stream, gw, gd, tiles_w, burst ? 1 : 0, fold);
    }
    if (i == 2 && e->variational) {
        if (!e->hooks.reparam_bwd) return fail(CAE_ERR_STATE, "trunk engine without a reparameterisation hook");
        e->hooks.reparam_bwd(e->hooks.user, e->stream, e->fptr(e->off_vgz), e->fptr(e->fc[1].act_off), B, e->latent,
                             e->fptr(e->fc[1].grad_off));
    }
    return CAE_OK;
}

// shape-generic: k_lin_wgrad, then k_lin_dgrad
void linear_bwd_generic(cae_engine* e, const StepArgs& a, int i, const ConvLayer& P) {
    const FcLayer& F = e->fc[i];
    const int B = a.batch, hw = P.hout * P.wout;
    hipStream_t s = e->stream;
    const float* gout = e->fptr(F.grad_off);
    const float* in = linear_in(e, i, P);
    BnDesc bni = i == 0 ? bn_of(e, P, BN_SAVED, 0, 0) : bn_none();
    {
        ProfScope _p(e, "linear_wgrad", i, f4((double)B * (F.nin + F.nout)) + 8.0 * F.nin * F.nout);
        hipLaunchKernelGGL(k_lin_wgrad, dim3(grid1((int64_t)F.nin * F.nout)), dim3(256),
                           lds_bytes(i == 0 ? P.cout : 0, 0), s, B, F.nin, F.nout, gout, in, bni, hw,
                           e->gradacc() + F.w_off, e->gradacc() + F.b_off);
    }
    ProfScope _p(e, "linear_dgrad", i, f4((double)B * (2.0 * F.nin + F.nout) + (double)F.nin * F.nout));
    if (i > 0) {
        const FcLayer& G = e->fc[i - 1];
        hipLaunchKernelGGL(k_lin_dgrad, dim3(grid1((int64_t)B * F.nin)), dim3(256), lds_bytes(0, 0), s, B,
                           F.nin, F.nout, gout, e->params + F.w_off, G.relu ? 1 : 0, e->fptr(G.act_off),
                           bn_none(), 1, (double*)nullptr, e->fptr(G.grad_off));
    } else {
        dim3 grid(grid1((int64_t)B * hw), P.cout);
        hipLaunchKernelGGL(k_lin_dgrad, grid, dim3(256), lds_bytes(P.cout, 0), s, B, F.nin, F.nout, gout,
                           e->params + F.w_off, 2, e->fptr(P.act_off), bni, hw, e->bn_stats(P.bn_index),
                           e->fptr(P.grad_off));
    }
}

// ---- backward: encoder convolutions ---------------------------------------------------------------------------------------------

// weight gradient and input gradient share only their inputs: one launch (kernels_generic.h k_conv_bwd_pair)
void enc_conv_bwd_pair(cae_engine* e, const StepArgs& a, const ConvBwd& c) {
    const ConvLayer& L = c.L;
    const int B = a.batch;
    const int64_t nw = (int64_t)L.cin * L.cout * L.kh * L.kw;
    const int64_t pos = (int64_t)B * L.hout * L.wout;
    WgradArgs wa = zeroed<WgradArgs>();
    wa.g = conv_geom(B, L); wa.small = c.gy; wa.bns = c.bng; wa.big = c.ain; wa.bnb = c.prod.bn_prev;
    wa.acc = e->gradacc() + L.w_off; wa.ppb = wgrad_ppb(pos, nw); wa.bg = bn_grad_out(e, L, a);
    UpArgs ua = zeroed<UpArgs>();
    ua.g = wa.g; ua.small = c.gy; ua.bns = c.bng; ua.w = e->params + L.w_off; ua.bias = nullptr;
    ua.e = epi_gin(c.prod); ua.bne = c.prod.bn_prev;
    const int nwy = (int)((pos + wa.ppb - 1) / wa.ppb), ux = grid1((int64_t)B * L.hin * L.win);
    ProfScope _p(e, "enc_conv_bwd_pair", c.l, f4((double)B * (3.0 * L.in_elems() + 4.0 * L.out_elems())));
    hipLaunchKernelGGL(k_conv_bwd_pair, dim3((unsigned)(nw * nwy + (int64_t)ux * L.cin)), dim3(256), lds_bytes(L.cout, L.cin), e->stream,
                       wa, ua, (int)nw, nwy, ux, (const StepState*)e->state());
}

// The first encoder layer's weight gradient, the last launch of backward, folds into the optimiser launch where
// enc_conv0_in_adam_ok holds (kernels_generic.h AdamConv0): nothing is launched here, launch_one hands c0_pending to k_adam.
void enc_conv0_into_adam(cae_engine* e, const StepArgs& a, const ConvBwd& c) {
    const ConvLayer& L = c.L;
    AdamConv0& c0 = e->c0_pending;
    c0.on = 1; c0.nw = L.cin * L.cout * L.kh * L.kw; c0.C = L.cout;
    c0.w_off = L.w_off; c0.gamma_off = L.gamma_off; c0.beta_off = L.beta_off;
    c0.g = conv_geom(a.batch, L); c0.small = c.gy; c0.bns = c.bng;
    c0.xb = e->fptr(e->off_xbatch);
    c0.bns.gamma = c0.xb + (int64_t)a.batch * L.in_elems();   // k_head_fwd's copy: this launch rewrites the parameter itself
    c0.stats = e->bn_stats(L.bn_index); c0.scale = 1.0;
}

// shape-generic: k_wgrad, then (behind a producer) the input gradient on k_up
void enc_conv_bwd_generic(cae_engine* e, const StepArgs& a, const ConvBwd& c) {
    const ConvLayer& L = c.L;
    const int B = a.batch;
    hipStream_t s = e->stream;
    const StepState* st = e->state();
    const ConvGeom g = conv_geom(B, L);
    {
        const int64_t nw = (int64_t)L.cin * L.cout * L.kh * L.kw;
        const int64_t pos = (int64_t)B * L.hout * L.wout;
        const int ppb = wgrad_ppb(pos, nw);
        dim3 grid((unsigned)nw, (unsigned)((pos + ppb - 1) / ppb));
        ProfScope _p(e, "enc_conv_wgrad", c.l, bytes_bwd(B, L, false, true), s);
        hipLaunchKernelGGL(k_wgrad, grid, dim3(256), lds_bytes(L.cout, L.cin), s, g, c.gy, c.bng, c.ain, c.prod.bn_prev,
                           e->gradacc() + L.w_off, ppb, bn_grad_out(e, L, a), st);
    }
    if (!c.prod.P) return;
    dim3 grid(grid1((int64_t)B * L.hin * L.win), L.cin);
    ProfScope _p(e, "enc_conv_dgrad", c.l, bytes_bwd(B, L, false, false));
    hipLaunchKernelGGL(k_up, grid, dim3(256), lds_bytes(L.cout, L.cin), s, g, c.gy, c.bng, e->params + L.w_off,
                       (const float*)nullptr, epi_gin(c.prod), c.prod.bn_prev, st);
}

}  // namespace
