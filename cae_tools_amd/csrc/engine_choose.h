// engine_choose.h - host only: every chooser and planner of the ConvAE step, and nothing that launches.  What these return is
// the whole decision: the launch code (engine_launch.h, engine_step.h) switches on it and cae_debug_plan, at the end of this
// file, reports it.
#pragma once

namespace {

// ---- specialised stride-2 kernels (kernels_s2.h): dispatch on (Cin, Cout, kh, kw) ----------------

#define S2_SHAPES(X) X(2, 1) X(4, 2) X(8, 4) X(6, 3)
#define S2_KERNELS(X, CI, CO) X(CI, CO, 3, 3) X(CI, CO, 4, 4) X(CI, CO, 3, 4) X(CI, CO, 4, 3)

template <int CI, int CO, int KH, int KW>
struct S2Shape { static constexpr int cin = CI, cout = CO, kh = KH, kw = KW; };

// Walks S2_SHAPES x S2_KERNELS in that order and hands L's shape, as an S2Shape, to fn; false: L's shape is not among them.
// The return types here and of the callers' lambdas are deduced, so both are instantiated where the caller stands and the
// kernel launchers they name are first used there: template kernels are emitted in the order of first use.
template <class F>
auto s2_for_shape(const ConvLayer& L, F fn) {
#define ONE(CI, CO, KH_, KW_) \
    if (L.cin == CI && L.cout == CO && L.kh == KH_ && L.kw == KW_) return fn(S2Shape<CI, CO, KH_, KW_>{});
#define PAIR(CI, CO) S2_KERNELS(ONE, CI, CO)
    S2_SHAPES(PAIR)
#undef PAIR
#undef ONE
    return false;
}

bool s2_shape_ok(const ConvLayer& L) { return L.transposed && L.stride == 2 && s2_for_shape(L, [](auto) { return true; }); }

bool s2_eligible(const cae_engine* e, const ConvLayer& L) { return e->use_s2 && L.sh_w >= 0 && s2_shape_ok(L); }

// ---- kernel choice of the decoder's conv-transposes ---------------------------------------------------------------------
// The choosers below (choose_s2_fwd / choose_s2_bwd / choose_rows_* / choose_last here, choose_dec_fwd / choose_dec_bwd after
// the fused head and tail) are the whole decision: the launch code switches on what they return and cae_debug_plan reports it.

// k_s2_fwd family.  tw: the tile width template argument.
enum S2FwdK {
    S2F_CS,     // small maps, many weights: k_s2_fwd_cs (output channels split over the waves)
    S2F_QUAD,   // small maps: k_s2_fwd (one quad per thread)
    S2F_WIDE    // k_s2_fwd2 (2x2 quads per thread)
};
struct S2FwdPick { S2FwdK k; int tw; };

S2FwdPick choose_s2_fwd(const ConvLayer& L, int B, int epi) {
    // each thread of k_s2_fwd2 covers 2x2 quads; lanes run along the row
    const int px = ((L.wout + 1) / 2 + 1) / 2, py = ((L.hout + 1) / 2 + 1) / 2;   // thread columns / rows per image
    if ((long long)B * px * py < 100000) {
        // small maps: 4x4 outputs per thread would leave most SIMDs without a wave; one quad per thread
        const int qx = (L.wout + 1) / 2;
        const int tw = qx > 32 ? 64 : 32;
        // intermediate layers with many weights: output channels split over the waves
        if (L.cin * L.cout * L.kh * L.kw > 80 && (256 / L.cout) % 64 == 0 && (epi == S2_RAW_STATS || epi == S2_RAW))
            return {S2F_CS, tw};
        return {S2F_QUAD, tw};
    }
    return {S2F_WIDE, px > 32 ? 64 : (px > 16 ? 32 : 16)};
}

// k_s2_bwd family.  tw: tile width (k_s2_bwd2); ct: input channels per thread (k_s2_bwd_split, k_s2_bwd).
enum S2BwdK {
    S2B_DIRECT,   // at most 72 weights: k_s2_bwd2 (one input pixel per thread, no LDS staging)
    S2B_SPLIT,    // 8 input channels, at most 72 weights per wave: k_s2_bwd_split (channels split over the 4 waves)
    S2B_GENERAL   // k_s2_bwd
};
struct S2BwdPick { S2BwdK k; int tw, ct; };

S2BwdPick choose_s2_bwd(const ConvLayer& L) {
    const int nw = L.cin * L.cout * L.kh * L.kw;
    if (nw <= 72) return {S2B_DIRECT, L.win > 32 ? 64 : 32, 0};
    if (L.cin == 8 && nw / 4 <= 72) return {S2B_SPLIT, 32, 2};
    return {S2B_GENERAL, 32, (L.cin % 2 == 0 && L.cin != 6) ? 2 : 3};
}

// grid caps of the k_s2_fwd family (k_s2_fwd / k_s2_fwd_cs, k_s2_fwd2), measured on MI355X at batch 64 (workgroups walk the
// remaining tiles): more workgroups only add fp64-atomic traffic at the end of the kernel
constexpr int kS2FwdCap = 1024, kS2Fwd2Cap = 512;
// ... and of k_s2_bwd2 / k_s2_bwd_split: each workgroup ends with Cin*Cout*kh*kw + 2*Cin fp64 atomics, and those dominate
// beyond 512 (measured per step at batch 64: 1536 -> 286 us, 512 -> 274 us)
constexpr int kS2BwdCap = 512;
// ... and of k_s2_bwd
constexpr int kS2BwdGeneralCap = 1024;

// ---- row-streaming backward of the thin middle layers (kernels_rows.h) ---------------------------------------------------
// false: the layer does not fit (shape, kernel size, map wider than a wave); the caller runs k_s2_bwd2 / k_s2_bwd_split
bool rows_bwd_ok(const cae_engine* e, const ConvLayer& L) {
    if (!s2_eligible(e, L) || L.kh != 3 || L.kw != 3 || !L.has_bn) return false;
    const int qw = (L.wout + 1) / 2;
    const int lw = qw <= 32 ? 32 : 64;
    if (qw > 64 || L.win > lw - 1) return false;      // a lane per quad column; the last lane of an image owns no pixel
    return (L.cin == 4 && L.cout == 2) || (L.cin == 8 && L.cout == 4);
}

// the variant of the row-streaming kernels: quad rows per band (HB), load depth (D, backward), lane width of an image (32: two
// images per wave, 64: one)
struct RowsPick { int hb, d, lw; };

int rows_lw(const ConvLayer& L) { return (L.wout + 1) / 2 <= 32 ? 32 : 64; }

RowsPick choose_rows_bwd(const ConvLayer& L) {
    // 4 -> 2: short bands with every row's loads issued up front (a wave pays the memory latency once); 8 -> 4: tall bands that
    // load one row ahead (less re-reading at the band edges, but a round trip per row: a wave is alone on its SIMD)
    return L.cin == 4 ? RowsPick{2, 3, rows_lw(L)} : RowsPick{4, 1, rows_lw(L)};
}

RowsPick choose_rows_fwd(const ConvLayer& L) { return RowsPick{L.cin == 4 ? 2 : 1, 0, rows_lw(L)}; }

// ---- last decoder layer of a training step as one launch (kernels_last.h): forward + sigmoid + MSE + backward ---------
bool last_fused_ok(const cae_engine* e, const ConvLayer& L) {
    return s2_eligible(e, L) && L.cin * L.cout * L.kh * L.kw <= 72 && L.sh_b >= 0;
}

// k_s2_last_fused: a wave walks a band of kLastHB quad rows (+1 recomputed): taller bands recompute less, shorter ones give more
// waves (measured at the benchmark geometry: 2048 waves of 4+1 rows, two per SIMD, beat 1024 of 8+1: 20.4 against 21.8 us;
// and at batch 128 / 512, where 8+1 rows used to be chosen: 244.2 against 246.8 and 601.6 against 607.6 us per step - the
// 8-row variant's register arrays end up in scratch)
constexpr int kLastHB = 4;

// the variant of k_s2_last_fused: 16-byte target loads (one strip, width a multiple of 4), BatchNorm on its input (a producer
// with BatchNorm)
struct LastPick { bool vec4, bn; };

int last_strips(const ConvLayer& L) {
    const int qw = (L.wout + 1) / 2;
    const int wmax = L.win > qw - 1 ? L.win : qw - 1;
    return (wmax + kLastStripPx - 1) / kLastStripPx;
}

LastPick choose_last(const ConvLayer& L, bool bn_in) { return LastPick{last_strips(L) == 1 && (L.wout & 3) == 0, bn_in}; }

// ---- LDS-staged implicit-GEMM forward of a channel-rich stride-2 ConvTranspose2d (kernels_ctlds.h) ---------------------
// ct_fwd_plan false: the layer does not fit this kernel (odd channel counts, kernels other than 3/4 taps, an image + weight
// slice larger than LDS); the layer then runs the gather kernel k_ig_fwd_s2.
// MFMAs per wave before K is split further
constexpr int kCtFwdMfmas = 24;

// Fills c's geometry and split; false: the layer does not fit (see above).
bool ct_fwd_plan(const cae_engine* e, int batch, const ConvLayer& L, int layer, CtFwd& c, int& waves, size_t& lds) {
    // Against the gather kernel it replaces (k_ig_fwd_s2) the LDS-staged one has a third of the instructions and wins from
    // batch 128 up (239.9 / 342.1 / 590.8 against 243.6 / 349.5 / 598.3 us per step at 128 / 256 / 512); at the benchmark's 64
    // both take 8-11 us per launch, all of it latency, and the step is 0.8 us shorter with the gather kernels (167.7 against
    // 168.5, four alternating runs) - but their gradients at that size sit 6.8e-4 from the oracle's where the LDS-staged
    // forward's sit within the full-size test's 2e-4 (test_full_size_gpu.py): parity first, the LDS-staged kernels run.
    if (e->gather_fwd || layer >= 31 || L.cin % 4 || L.kh < 3 || L.kw < 3) return false;
    memset(&c, 0, sizeof c);
    c.B = batch; c.Cin = L.cin; c.H = L.hin; c.W = L.win; c.Cout = L.cout; c.OH = L.hout; c.OW = L.wout;
    c.QH = (L.hout + 1) / 2; c.QW = (L.wout + 1) / 2;
    c.PW = c.QW + 1;
    c.inv_qw = 1.0f / (float)c.QW; c.inv_w = 1.0f / (float)c.W;
    c.tiles = (c.QH * c.QW + 15) / 16;
    const int taps = ((L.kh + 1) / 2 + L.kh / 2) * ((L.kw + 1) / 2 + L.kw / 2);   // sum of n_p over the four parities = kh * kw
    const int mf = L.cin * taps / 4;
    int ks = 1;
    while (ks < 8 && mf / ks > kCtFwdMfmas && L.cin % (ks * 2 * 4) == 0) ks *= 2;
    int rt = 8 / ks;
    if (rt > c.tiles) rt = c.tiles;
    if (rt > 4) rt = 4;
    c.ks = ks; c.rt = rt;
    c.tg = (c.tiles + rt - 1) / rt;
    waves = rt * ks;
    // A workgroup stages the band of input rows its tile group reads, (first quad row - 1) .. last quad row: the LDS plane
    // holds the tallest band of the image.  Which layers take this kernel is still decided on the whole padded image, as it
    // was when every workgroup staged it (the splits above were only measured on maps that small).
    int brows = 0;
    for (int g = 0; g < c.tg; g++) {
        const int qs = g * rt * 16, qe = std::min(qs + rt * 16, c.QH * c.QW);
        brows = std::max(brows, (qe - 1) / c.QW - qs / c.QW + 2);
    }
    c.plane = (brows * c.PW) | 1;
    const int whole = ((c.QH + 1) * c.PW) | 1;
    lds = ct_fwd_lds_bytes(L.cin, c.plane, L.kh, L.kw, waves, ks);
    return !(ct_fwd_lds_bytes(L.cin, whole, L.kh, L.kw, waves, ks) > 150 * 1024 || whole >= kDivSmallMaxD ||
             (long long)L.cin * whole >= kDivSmallMaxN);
}

// ---- LDS-staged backward of a channel-rich stride-2 ConvTranspose2d (kernels_ctbwd.h, the kernels in ctbwd.hip) ----------
// The layers of cae_set_kernel_mode's mask with 3x3 kernels at stride 2, whole 16-channel blocks, images that fit the staging
// registers / LDS, and few enough images per accumulator address.  False: the gather pair k_ig_bwd_pair.
// The launch: grid (groups, Cin / 16, parts) with lds_launch bytes; bands > 1: the band kernel, bands of hb input rows.
struct CtBwdPlan { int imgs, groups, wstr; size_t lds; int parts, bands, hb; size_t lds_launch; };

// LDS of k_ct_bwd_lds with imgs whole images staged: mirrors the carve of ct_bwd_body<false> (kernels_ctbwd.h, ct_bwd_lds_bytes)
size_t ct_bwd_whole_lds(const ConvLayer& L, int imgs, int wstr) {
    return ct_bwd_lds_bytes(L.cin, L.cout, imgs, L.hin * L.win, L.hout * L.wout, wstr);
}

// LDS of k_ct_bwd_band with a band of hb input rows (2 hb + 1 gradient rows) staged: mirrors the carve of ct_bwd_body<true>
size_t ct_bwd_band_lds(const ConvLayer& L, int hb, int wstr) {
    const int gstr = (2 * hb + 1) * L.wout, astr = hb * L.win;
    return (32 * (size_t)kCtbWaves + 4 * (size_t)(L.cin + L.cout) + (size_t)L.cout * gstr + 4 + 16 * (size_t)astr + 4 +
            16 * (size_t)wstr + 3 * (size_t)astr + (size_t)kCtbWaves * 16 * 17 + 8) * sizeof(float);
}

// how the workgroups of a layer that fits (imgs, groups, wstr, lds set) split the image: ~256 workgroups
void ct_bwd_band_plan(const ConvLayer& L, CtBwdPlan& p) {
    p.parts = std::max(1, std::min(8, 256 / (p.groups * (L.cin / 16))));
    p.bands = p.hb = 0; p.lds_launch = p.lds;
    if (p.imgs == 1 && p.parts > 1) {
        // one image per workgroup and workgroups to spare: bands of input rows instead of workgroups that
        // stage the same image (where the band's pieces fit the band kernel's staging registers)
        const int hb = (L.hin + p.parts - 1) / p.parts, bands = (L.hin + hb - 1) / hb;
        const int gstr = (2 * hb + 1) * L.wout, astr = hb * L.win;
        if (bands > 1 && L.cout * gstr <= 8 * kCtbThreads && 16 * astr <= 2 * kCtbThreads) {
            p.bands = p.parts = bands; p.hb = hb;
            p.lds_launch = ct_bwd_band_lds(L, hb, p.wstr);
        }
    }
}

bool ct_bwd_plan(const cae_engine* e, int B, const ConvLayer& L, int l, CtBwdPlan& p) {
    if (!(l < 31 && ((e->ctbwd_mask >> l) & 1) && L.kh == 3 && L.kw == 3 && L.stride == 2 && L.cin % 16 == 0 && L.cout % 4 == 0 &&
          L.hout >= 2 * L.hin + 1 && L.wout >= 2 * L.win + 1))
        return false;
    const int HW = L.hin * L.win, OHW = L.hout * L.wout, N = L.cout * 9;
    const int budget = std::min((4 * kCtbG4 * kCtbThreads) / (L.cout * OHW), (4 * kCtbA4 * kCtbThreads) / (16 * HW));
    int imgs = (int)(((int64_t)L.cin * N * B + 149999) / 150000);
    imgs = std::max(1, std::min(std::min(imgs, budget), B));
    p.imgs = imgs;
    p.groups = (B + imgs - 1) / imgs;
    p.wstr = N | 1;
    p.lds = ct_bwd_whole_lds(L, imgs, p.wstr);
    ct_bwd_band_plan(L, p);
    return budget >= 1 && 16 * N <= 4 * kCtbW4 * kCtbThreads && p.lds <= 152 * 1024 && (int64_t)L.cin * N * p.groups <= 400000;
}

// ---- gather kernels of the channel-rich layers (kernels_igemm.h) ---------------------------------------------------------
// k_ig_fwd_s2: K split over the waves, row tiles per wave, grid and LDS
struct IgFwdPlan { int ksplit, tiles_per_wave; dim3 grid; size_t lds; };

IgFwdPlan ig_fwd_plan(const ConvLayer& L, int B) {
    IgFwdPlan p;
    const int mtiles = (B * ((L.hout + 1) / 2) * ((L.wout + 1) / 2) + 15) / 16;
    p.ksplit = L.cin >= 48 ? 4 : (L.cin >= 24 ? 2 : 1);
    // at most ~1024 workgroups over the 4 parities: every workgroup ends with up to 32 fp64 atomics
    const int waves_m = 4 / p.ksplit, target = 1024;
    const int tpw = (mtiles * 4 + waves_m * target - 1) / (waves_m * target);
    p.tiles_per_wave = tpw < 1 ? 1 : (tpw > 8 ? 8 : tpw);
    const int per_block = waves_m * p.tiles_per_wave;
    p.grid = dim3((mtiles + per_block - 1) / per_block, 4, (L.cout + 15) / 16);
    p.lds = (64 + 1024) * sizeof(float) + (size_t)(L.cin + 1) * sizeof(float4);
    return p;
}

// k_ig_bwd_pair: the weight-gradient half (wtiles tiles x chunks of `per` k-steps), the input-gradient half (d_gx x d_gy blocks,
// K split over the waves) and the XCD-aware block order that interleaves them
struct IgBwdPlan { int wtiles, chunks, per, ksplit, tiles_per_wave, d_gx, d_gy, d_group, w_n8; unsigned grid; size_t lds; };

IgBwdPlan ig_bwd_plan(const ConvLayer& L, int B) {
    IgBwdPlan p;
    p.wtiles = ((L.cin + 15) / 16) * ((L.cout * L.kh * L.kw + 15) / 16);
    const int steps = (B * L.hin * L.win + 3) / 4;
    const int chunks = std::max(1, 2048 / p.wtiles);   // ~2048 weight-gradient workgroups
    p.per = ((steps + chunks - 1) / chunks + 31) / 32 * 32;
    p.chunks = (steps + p.per - 1) / p.per;
    const int mtiles = (B * L.hin * L.win + 15) / 16;
    const int ksteps = (L.cout * L.kh * L.kw + 3) / 4;
    p.ksplit = ksteps > 24 ? 4 : (ksteps > 12 ? 2 : 1);   // <= 12 k-steps (one load batch) per wave where possible
    p.tiles_per_wave = mtiles >= 8192 ? 2 : 1;
    const int per_block = (4 / p.ksplit) * p.tiles_per_wave;
    p.d_gx = (mtiles + per_block - 1) / per_block;
    p.d_gy = (L.cin + 15) / 16;
    const size_t lds_d = (128 + 1024) * sizeof(float) + (size_t)(L.cin + L.cout + 1) * sizeof(float4) +
                         (size_t)L.cout * L.kh * L.kw * 2 * sizeof(int);
    const size_t lds_w = 1024 * sizeof(float) + (size_t)(L.cin + L.cout + 1) * sizeof(float4);
    p.lds = lds_d > lds_w ? lds_d : lds_w;
    // XCD-aware order (kernels_igemm.h): d_group input-gradient blocks cover the positions of one weight-gradient chunk
    p.d_group = std::max(1, (p.per * 4) / (per_block * 16));
    p.w_n8 = (p.chunks + 7) / 8;
    const int d_n8 = ((p.d_gx + p.d_group - 1) / p.d_group + 7) / 8;
    p.grid = (unsigned)(8 * p.wtiles * p.w_n8 + 8 * d_n8 * p.d_group * p.d_gy);
    return p;
}

// ---- fused head / tail (kernels_head.h) ----------------------------------------------------------

// `floats` more of an LDS layout that ends at top: their offset, in floats and 16-byte aligned
int lds_take(int64_t& top, int64_t floats) {
    const int64_t o = align_up(top, 4);
    top = o + floats;
    return (int)o;
}

// Fills the descriptor shared by k_head_fwd and k_tail_bwd and lays out their LDS.  Returns false when the model or
// the batch does not fit (the caller then runs the per-layer launches); *why then names the first condition that failed
// (cae_debug_plan reports it).
bool head_plan(const cae_engine* e, const StepArgs& a, HeadArgs& h, size_t& lds_bytes, const char** why = nullptr) {
    auto no = [&](const char* reason) {
        if (why) *why = reason;
        return false;
    };
    if (!e->use_s2) return no("mode");
    if (a.syncing()) return no("syncing");
    if (e->variational) return no("variational");
    if ((int)e->enc.size() > kHeadMaxEnc) return no("depth");
    memset(&h, 0, sizeof h);
    h.B = a.batch;
    h.n_enc = (int)e->enc.size();
    h.train = a.train ? 1 : 0;
    h.momentum = kBnMomentum;
    h.eps = kBnEps;
    h.st = e->state();
    // Linear-3 column tiles per workgroup (1 since the end of round 2: 168.2 against 169.7 us per step with 4 - more workgroups
    // recompute the encoder, each holds a quarter of the last Linear layer's weights and finishes its strip sooner; 8: 186.9)
    h.tiles_per_wg = 1;
    double* acc = e->gradacc();
    int64_t top = 0;
    auto take = [&](int64_t floats) { return lds_take(top, floats); };
    h.o_perm = take(a.batch);
    int maxc = 1;
    for (int l = 0; l < h.n_enc; l++) {
        const ConvLayer& L = e->enc[l];
        if (L.cout > kHeadMaxC) return no("channels");
        HeadConv& c = h.enc[l];
        c.cin = L.cin; c.hin = L.hin; c.win = L.win; c.cout = L.cout; c.hout = L.hout; c.wout = L.wout;
        c.kh = L.kh; c.kw = L.kw; c.s = L.stride;
        c.w = e->params + L.w_off; c.bias = e->params + L.b_off;
        c.gamma = e->params + L.gamma_off; c.beta = e->params + L.beta_off;
        c.rmean = e->bufs + L.rm_off; c.rvar = e->bufs + L.rv_off; c.saved = e->bn_saved(L.bn_index);
        c.y = e->fptr(L.act_off);
        {
            const double count = (double)a.batch * L.hout * L.wout;
            c.inv_count = 1.0 / count;
            c.unbias = count > 1.0 ? count / (count - 1.0) : 1.0;
        }
        {   // two burst segments: [conv weight .. BatchNorm bias] of the parameter arena, [running mean .. var] of the buffers
            const int64_t pn = L.beta_off + L.cout - L.w_off, bnn = L.rv_off + L.cout - L.rm_off;
            if (pn > kHeadThreads || bnn > kHeadThreads || pn <= 0 || bnn <= 0) return no("params");
            if (h.n_seg + 2 > kHeadMaxSeg) return no("segments");
            c.o_w = take(pn);
            c.o_b = c.o_w + (int)(L.b_off - L.w_off);
            c.o_gamma = c.o_w + (int)(L.gamma_off - L.w_off);
            c.o_beta = c.o_w + (int)(L.beta_off - L.w_off);
            c.o_rm = take(bnn);
            c.o_rv = c.o_rm + (int)(L.rv_off - L.rm_off);
            h.seg[h.n_seg++] = HeadSeg{e->params + L.w_off, (int)pn, c.o_w, 0};
            h.seg[h.n_seg++] = HeadSeg{e->bufs + L.rm_off, (int)bnn, c.o_rm, 0};
        }
        c.o_c = take(4 * (int64_t)L.cout);
        if (l + 1 == h.n_enc) c.o_y = take((int64_t)a.batch * L.out_elems());   // inner maps live in the union region
        if (L.cout > maxc) maxc = L.cout;
    }
    int maxd = 0;
    for (int i = 0; i < 4; i++) {
        const FcLayer& F = e->fc[i];
        HeadFc& f = h.fc[i];
        f.nin = F.nin; f.nout = F.nout; f.relu = F.relu ? 1 : 0;
        f.w = e->params + F.w_off; f.bias = e->params + F.b_off;
        f.act = e->fptr(F.act_off); f.grad = e->fptr(F.grad_off);
        f.w_acc = acc + F.w_off; f.b_acc = acc + F.b_off;
        if (i < 3 && F.nout > maxd) maxd = F.nout;
        if (i < 3 && F.nin > maxd) maxd = F.nin;
    }
    h.ld_h = (maxd + 31) / 32 * 32 + 2;   // row stride = 2 mod 32 banks: the 16 rows x 2 k of an MFMA operand read do not collide
    h.o_red = take(2 * 2 * (int64_t)maxc * kHeadWaves);   // doubles
    h.o_h[0] = take(16 * (int64_t)h.ld_h);
    h.o_h[1] = take(16 * (int64_t)h.ld_h + 32);   // + guard: an 8-deep k-batch may read up to 30 floats past row 15 (against zero B operands)
    h.o_part = take(kHeadWaves * 256);
    {   // union region: the gathered input and the encoder's inner maps while the encoder runs, the Linear weights after
        // (row stride = 4 mod 32 floats: 16-byte aligned rows, two-way bank conflicts at worst on the operand reads)
        int64_t wf = 0;
        int start4 = 0;
        for (int i = 0; i < 4; i++) {
            const FcLayer& F = e->fc[i];
            if (F.nin % 4) return no("nin4");   // whole k-steps and 16-byte rows
            const int rows = i == 3 ? 16 * h.tiles_per_wg : (F.nout + 15) / 16 * 16;
            HeadW& w = h.wmat[i];
            w.src = e->params + F.w_off;
            w.n4row = F.nin / 4;
            w.ldw = (F.nin + 31) / 32 * 32 + 4;
            w.start4 = start4;
            w.strip_floats = i == 3 ? 16 * h.tiles_per_wg * F.nin : 0;
            w.lds_off = (int)wf;   // relative, rebased below
            start4 += (i == 3 ? std::min(rows, F.nout) : F.nout) * w.n4row;
            wf += (int64_t)rows * w.ldw;
        }
        wf += 64;   // k-batches read past the last row
        h.w_total4 = start4;
        if (h.w_total4 > kHeadW4 * kHeadThreads) return no("weights");
        for (int j = 0; j < kHeadW4; j++) {
            const int lo = j * kHeadThreads, hi = std::min((j + 1) * kHeadThreads, h.w_total4) - 1;   // float4s of piece j
            h.piece_m[j] = -1;
            for (int m = 0; m < 4 && hi >= lo; m++) {
                const int mend = m < 3 ? h.wmat[m + 1].start4 : h.w_total4;
                if (lo >= h.wmat[m].start4 && hi < mend) h.piece_m[j] = m;
            }
        }
        int64_t ef = (int64_t)a.batch * e->enc[0].in_elems();
        for (int l = 0; l + 1 < h.n_enc; l++) ef += align_up((int64_t)a.batch * e->enc[l].out_elems(), 4);
        const int base = take(std::max(wf, ef));
        h.o_x = base;
        int64_t o = base + (int64_t)a.batch * e->enc[0].in_elems();
        for (int l = 0; l + 1 < h.n_enc; l++) {
            o = align_up(o, 4);
            h.enc[l].o_y = (int)o;
            o += (int64_t)a.batch * e->enc[l].out_elems();
        }
        for (int i = 0; i < 4; i++) h.wmat[i].lds_off += base;
    }
    for (int i = 0; i < 4; i++) {
        const int cnt = i == 3 ? 16 * h.tiles_per_wg : e->fc[i].nout;
        if (cnt > kHeadThreads) return no("biases");
        if (h.n_seg + 1 > kHeadMaxSeg) return no("segments");
        h.o_bias[i] = take(cnt);
        // Linear 3: a strip of 16 * tiles_per_wg biases per workgroup column; the last strip may read past the vector
        // (clamped reads inside the parameter arena, masked by the epilogue's n < N)
        h.seg[h.n_seg++] = HeadSeg{e->params + e->fc[i].b_off, i == 3 ? std::min(cnt, e->fc[3].nout) : cnt, h.o_bias[i], i == 3 ? 1 : 0};
    }
    for (int i = 0; i < 4; i++) {
        if (e->fc[i].nin % 4) return no("nin4");   // stage_prefetch walks whole k-steps
        const int tiles = i == 3 ? h.tiles_per_wg : (e->fc[i].nout + 15) / 16;
        h.fc_split[i] = stage_split(tiles, e->fc[i].nin);
    }
    lds_bytes = (size_t)align_up(top, 4) * sizeof(float);
    return lds_bytes <= 152 * 1024 || no("lds");
}


// k_tail_bwd (kernels_head.h): Linear 2..0 backward in one launch.  False: run the per-layer pair launches; *why then names
// the first condition that failed.
bool tail_plan(const cae_engine* e, const StepArgs& a, TailArgs& t, size_t& lds_bytes, const char** why = nullptr) {
    auto no = [&](const char* reason) {
        if (why) *why = reason;
        return false;
    };
    if (!e->use_s2) return no("mode");
    if (a.syncing()) return no("syncing");
    if (e->variational) return no("variational");
    memset(&t, 0, sizeof t);
    const ConvLayer& P = e->enc.back();
    double* acc = e->gradacc();
    t.B = a.batch;
    for (int i = 0; i < 3; i++) {
        const FcLayer& F = e->fc[i];
        if (F.nin % 4 || F.nout % 4) return no("fc4");              // 16-byte rows, whole k-steps
        if (16 * F.nout / 4 > 2 * kHeadThreads) return no("panel");   // a 16-row panel in two loads per thread
        HeadFc& f = t.fc[i];
        f.nin = F.nin; f.nout = F.nout; f.relu = F.relu ? 1 : 0;
        f.w = e->params + F.w_off; f.bias = e->params + F.b_off;
        f.act = e->fptr(F.act_off); f.grad = e->fptr(F.grad_off);
        f.w_acc = acc + F.w_off; f.b_acc = acc + F.b_off;
        t.w4[i] = F.nin * F.nout / 4;
        if (t.w4[i] > 2 * kHeadThreads) return no("weights");
        const int r16 = (F.nin + 15) / 16 * 16;
        t.ldw[i] = r16 % 32 == 0 ? r16 + 16 : r16;   // = 16 mod 32: the four k rows of an operand read land on distinct banks
    }
    if (P.cout > kHeadMaxC || e->fc[0].nin != P.cout * P.hout * P.wout) return no("channels");
    t.y_last = e->fptr(P.act_off);
    t.g_last = e->fptr(P.grad_off);
    t.gamma = e->params + P.gamma_off;
    t.beta = e->params + P.beta_off;
    t.saved = e->bn_saved(P.bn_index);
    t.stats = e->bn_stats(P.bn_index);
    t.C = P.cout;
    t.hw = P.hout * P.wout;
    auto ld_of = [](int n) { return (n + 31) / 32 * 32 + 4; };
    t.ld2 = ld_of(e->fc[2].nout);
    t.ld1 = ld_of(e->fc[1].nout);
    t.ld0 = ld_of(e->fc[0].nout);
    int64_t top = 0;
    auto take = [&](int64_t floats) { return lds_take(top, floats); };
    t.o_c = take(4 * (int64_t)P.cout);
    t.o_red = take(2 * 2 * (int64_t)kHeadWaves);
    t.o_g2 = take(16 * (int64_t)t.ld2 + 32);   // + guard: a k-batch may read a few floats past row 15 (against zero B operands)
    t.o_g1 = take(16 * (int64_t)t.ld1 + 32);
    t.o_g0 = take(16 * (int64_t)t.ld0 + 32);
    // y and gx sit inside the cleared region too: the weight-gradient stage reads all 16 panel rows without predicates, and
    // rows past the batch must be finite (they meet zero gradient rows; LDS garbage could be NaN)
    t.o_y = take(16 * (int64_t)e->fc[0].nin + 32);
    t.o_gx = take(16 * (int64_t)e->fc[0].nin + 32);
    top = align_up(top, 4);
    t.zero4 = (int)((top - t.o_g2) / 4);
    int64_t wmax = 0;
    for (int i = 0; i < 3; i++) wmax = std::max<int64_t>(wmax, (int64_t)e->fc[i].nout * t.ldw[i]);
    t.o_w = take(wmax + 64);
    t.o_part = take(kHeadWaves * 256);
    lds_bytes = (size_t)align_up(top, 4) * sizeof(float);
    if (lds_bytes > 152 * 1024) return no("lds");
    // chain (16 rows): g1 (N = fc2.nin, K = fc2.nout), g0 (N = fc1.nin, K = fc1.nout), gx (N = fc0.nin, K = fc0.nout)
    for (int i = 0; i < 3; i++) t.sp_d[i] = stage_split((e->fc[2 - i].nin + 15) / 16, e->fc[2 - i].nout);
    // weight-gradient shares: M = nout, N = nin + 1, K = 16 rows
    for (int i = 0; i < 3; i++) t.sp_w[i] = stage_split(((e->fc[2 - i].nout + 15) / 16) * ((e->fc[2 - i].nin + 16) / 16), 16);
    return true;
}

// ---- kernel choice of a decoder layer (see choose_s2_fwd above) ---------------------------------------------------------
enum DecFwdK {
    DF_FUSED_LAST,   // training step's last layer: nothing here, k_s2_last_fused runs forward, loss and backward in launch_backward
    DF_ROWS,         // k_s2_fwd_rows
    DF_S2,           // the k_s2_fwd family (choose_s2_fwd)
    DF_CT_LDS,       // k_ct_fwd_lds
    DF_IG,           // k_ig_fwd_s2
    DF_UP            // k_up (shape-generic)
};
enum DecBwdK {
    DB_FUSED_LAST,   // k_s2_last_fused
    DB_ROWS,         // k_s2_bwd_rows
    DB_S2,           // the k_s2_bwd family (choose_s2_bwd)
    DB_CT_LDS,       // k_ct_bwd_lds (ctbwd.hip)
    DB_IG,           // k_ig_bwd_pair
    DB_GENERIC       // k_wgrad + k_down (shape-generic)
};

// the k_s2_fwd epilogue of decoder layer L (layer l) in a step
int s2_fwd_epi(const cae_engine* e, int l, bool train, bool external_loss) {
    if (l + 1 < (int)e->dec.size()) return train ? S2_RAW_STATS : S2_RAW;
    if (external_loss) return S2_RAW;
    return train ? S2_SIGMSE : S2_SIGOUT;
}

// the thin middle layers behind a BatchNorm'd producer: the row-streaming kernels (forward and backward) where they fit
bool rows_ok(const cae_engine* e, const ConvLayer& L, int l) {
    return l + 1 < (int)e->dec.size() && l > 0 && e->dec[l - 1].has_bn && rows_bwd_ok(e, L);
}

DecFwdK choose_dec_fwd(const cae_engine* e, const ConvLayer& L, int l, int B, bool train, bool external_loss) {
    const bool last = l + 1 == (int)e->dec.size();
    if (last && train && !external_loss && last_fused_ok(e, L)) return DF_FUSED_LAST;
    if (rows_ok(e, L, l)) return DF_ROWS;
    if (s2_eligible(e, L)) return DF_S2;
    if (e->use_s2 && !last && L.stride == 2 && L.kh <= 4 && L.kw <= 4) {
        CtFwd c;
        int waves = 0;
        size_t lds = 0;
        return ct_fwd_plan(e, B, L, l, c, waves, lds) ? DF_CT_LDS : DF_IG;
    }
    return DF_UP;
}

DecBwdK choose_dec_bwd(const cae_engine* e, const ConvLayer& L, int l, int B, bool external_loss) {
    const bool last = l + 1 == (int)e->dec.size();
    if (last && !external_loss && last_fused_ok(e, L)) return DB_FUSED_LAST;
    if (rows_ok(e, L, l)) return DB_ROWS;
    if (s2_eligible(e, L)) return DB_S2;
    if (e->use_s2) {
        CtBwdPlan p;
        return ct_bwd_plan(e, B, L, l, p) ? DB_CT_LDS : DB_IG;
    }
    return DB_GENERIC;
}

// ---- weight-gradient partial slabs (folded by k_gemm16_pair: kernels_gemm.h wgrad_fold_body) -------------------------------
// A decoder backward kernel stores its weight-gradient partials instead of adding them where the step has the launch that
// folds them: launch_backward runs linear_bwd_pair(e, a, 3, P) behind the decoder whenever the specialised kernels are on,
// in every kind of step (single device, data-parallel, SyncBN, trunk).  cae_set_kernel_mode bit 3 keeps the atomics.
bool wgrad_slabs_on(const cae_engine* e) { return e->use_s2 && !e->wgrad_atomics; }

// One slab: slab[nparts][nvals] at `off` bytes of the region, for the weight of decoder layer `layer`.
//   k_ct_bwd_lds / k_ct_bwd_band (float: MFMA tiles): one partial per workgroup and chunk of kCtbKChunk positions.  Only the
//     last band of an image / the last image group is short, so the partials are numbered without gaps - band kernel (grid x =
//     image, z = band): x * ppg + z * kfull + chunk; whole images (grid x = image group): x * kfull + chunk
//   k_s2_bwd_rows (double: the four-wave sums): one partial per workgroup
// The weight-gradient half of k_ig_bwd_pair and k_s2_last_fused keep their atomics: as slab writers they were measured and
// did not pay.
struct WSlab { int layer; const char* writer; int nvals, nparts, f64, kfull, ppg; int64_t off; };

void ct_bwd_slab(const ConvLayer& L, const CtBwdPlan& p, int B, WSlab& s) {
    auto chunks = [](int positions) { return (positions + kCtbKChunk - 1) / kCtbKChunk; };
    s.nvals = L.cin * L.cout * 9;
    s.f64 = 0;
    if (p.bands > 1) {
        s.writer = "ct_bwd_band";
        s.kfull = chunks(p.hb * L.win);
        s.ppg = (p.bands - 1) * s.kfull + chunks((L.hin - (p.bands - 1) * p.hb) * L.win);
        s.nparts = p.groups * s.ppg;
    } else {
        s.writer = "ct_bwd_lds";
        s.kfull = s.ppg = chunks(p.imgs * L.hin * L.win);
        s.nparts = (p.groups - 1) * s.kfull + chunks((B - (p.groups - 1) * p.imgs) * L.hin * L.win);
    }
}

// the grid of rows_go (engine_launch.h)
int rows_bwd_grid(const ConvLayer& L, int B) {
    const RowsPick p = choose_rows_bwd(L);
    const int qh = (L.hout + 1) / 2, hmax = L.hin > qh - 1 ? L.hin : qh - 1, nb = L.cin == 4 ? 4 : 1;
    const int bands = (hmax + p.hb - 1) / p.hb, imgs = 64 / p.lw;
    return ((B + imgs - 1) / imgs) * ((bands + nb - 1) / nb);
}

// The slabs of a training step at batch B in launch order (last decoder layer first): every layer whose backward kernel is a
// slab writer, while the fold launch has room (kFoldMax slabs, `capacity` bytes; a layer beyond keeps its atomics).
std::vector<WSlab> wgrad_slab_table(const cae_engine* e, int B, bool external_loss, int64_t capacity) {
    std::vector<WSlab> t;
    if (!wgrad_slabs_on(e)) return t;
    int64_t used = 0;
    for (int l = (int)e->dec.size() - 1; l >= 0; l--) {
        const ConvLayer& L = e->dec[l];
        WSlab s{l, "", L.cin * L.cout * L.kh * L.kw, 0, 1, 0, 0, 0};
        switch (choose_dec_bwd(e, L, l, B, external_loss)) {
            case DB_ROWS:
                s.writer = "s2_bwd_rows"; s.nparts = rows_bwd_grid(L, B);
                break;
            case DB_CT_LDS: {
                CtBwdPlan p;
                (void)ct_bwd_plan(e, B, L, l, p);
                ct_bwd_slab(L, p, B, s);
                break;
            }
            default: continue;
        }
        const int64_t bytes = align_up((int64_t)s.nparts * s.nvals * (s.f64 ? 8 : 4), 256);
        if ((int)t.size() >= kFoldMax || used + bytes > capacity) continue;
        s.off = used;
        used += bytes;
        t.push_back(s);
    }
    return t;
}

// layer l's slab in the table of the step at hand (nparts == 0: none, the layer adds with atomics)
WSlab wgrad_slab_of(const cae_engine* e, int B, bool external_loss, int l) {
    for (const WSlab& s : wgrad_slab_table(e, B, external_loss, e->wslab_bytes))
        if (s.layer == l) return s;
    return WSlab{l, "", 0, 0, 0, 0, 0, 0};
}

// bytes of the slab region: the most a step of any batch up to max_batch stores, with every eligible layer on the
// LDS-staged backward (cae_set_kernel_mode bit 1)
int64_t wgrad_slab_capacity(cae_engine* e) {
    const int mask = e->ctbwd_mask;
    e->ctbwd_mask = 0x7fffffff;
    int64_t cap = 0;
    for (int B = 1; B <= e->max_batch; B++) {
        const std::vector<WSlab> t = wgrad_slab_table(e, B, e->variational, INT64_MAX / 2);
        if (!t.empty()) cap = std::max(cap, t.back().off + align_up((int64_t)t.back().nparts * t.back().nvals * (t.back().f64 ? 8 : 4), 256));
    }
    e->ctbwd_mask = mask;
    return cap;
}

// the fold section of Linear 3's backward launch for that table
WFold wgrad_fold_of(const cae_engine* e, const std::vector<WSlab>& t) {
    WFold f = zeroed<WFold>();
    for (const WSlab& s : t) {
        const int vshift = fold_vshift(s.nparts);
        f.s[f.nslab++] = WFoldSlab{e->ws + e->off_wslab + s.off, e->gradacc() + e->dec[s.layer].w_off, s.nvals, s.nparts, s.f64, vshift};
        f.nwg += fold_wgs(s.nvals, vshift);
    }
    return f;
}

// The first encoder layer's weight gradient inside the optimiser launch (kernels_generic.h AdamConv0): a single-device training step
// whose k_head_fwd left the batch's inputs behind, a layer small enough for k_adam's extra blocks, its BatchNorm table first in the swept range.
// enc_conv0_fits_adam: what the engine and the layer decide (cae_debug_plan reports it for a step with a fused head);
// enc_conv0_in_adam_ok adds the two facts of the step at hand: the optimiser follows, k_head_fwd published the inputs
// (the per-weight workgroups' index arithmetic, adam_conv0_body: small divisors, 24-bit factors, 32-bit byte offsets)
bool enc_conv0_fits_adam(const cae_engine* e, const StepArgs& a, const ConvLayer& L) {
    return e->use_s2 && !a.syncing() && a.world == 1 && L.cout <= 64 &&
           (int64_t)L.cin * L.cout * L.kh * L.kw <= 4096 && (int64_t)a.batch * L.hout * L.wout < kDivSmallMaxN &&
           L.hout * L.wout < kDivSmallMaxD && L.in_elems() < (1 << 24) && L.out_elems() < (1 << 24) &&
           (int64_t)a.batch * L.in_elems() < (1 << 30) && (int64_t)a.batch * L.out_elems() < (1 << 30) &&
           e->bn_stat_off[L.bn_index] == e->off_zero_begin;
}

bool enc_conv0_in_adam_ok(const cae_engine* e, const StepArgs& a, const ConvLayer& L) {
    return a.adam_follows && e->x_published && enc_conv0_fits_adam(e, a, L);
}

// The input-gradient GEMM of Linear i's backward pair (linear_bwd_pair: gin[b][:] = gout[b][:] W, contraction over the layer's
// nout outputs, gout rows nout floats apart) on the burst variant of k_gemm16_pair (kernels_gemm.h gemm16_burst_body): every
// operand read issued at kernel start.  It needs 16-byte rows of gout (nout a multiple of 4), at most kBurstSteps k-steps per
// wave, and pays from 128 outputs on; Linear 0's input gradient carries the BatchNorm mask epilogue, which it does not have.
bool linear_bwd_burst(const cae_engine* e, int i) {
    const int K = e->fc[i].nout;
    return i > 0 && K % 4 == 0 && K >= 128 && (K / 4 + 3) / 4 <= kBurstSteps;
}

// how head_stage_inputs (kernels_head.h) brings the batch to LDS without a permutation: one contiguous block of 16-byte loads,
// 16-byte loads through the sample table, or scalar loads (inputs per sample no multiple of 4)
const char* head_staging(const HeadArgs& h) {
    const int per = h.enc[0].cin * h.enc[0].hin * h.enc[0].win;
    if (per & 3) return "scalar";
    return h.B * (per >> 2) <= 4 * kHeadThreads ? "direct" : "gather4";
}

}  // namespace

extern "C" {

int cae_debug_plan(const cae_engine* e, int batch, int train, char* out, int64_t out_bytes) {
    if (!e || !out || out_bytes < 1) return fail(CAE_ERR_ARG, "cae_debug_plan: bad argument");
    if (batch < 1 || batch > e->max_batch) return fail(CAE_ERR_ARG, "cae_debug_plan: batch %d outside 1 .. %d", batch, e->max_batch);
    // the step of a single device without SyncBN; the trunk of the var engine hands its last layer's raw output to a loss outside
    const bool tr = train != 0, ext = e->variational;
    const StepArgs a{0, nullptr, batch, batch, batch, tr, true, nullptr, nullptr, false};
    std::string s;
    char line[512];
    bool head_fused = false;
    {
        HeadArgs h;
        size_t lds = 0;
        const char* why = "";
        head_fused = head_plan(e, a, h, lds, &why);
        if (head_fused) {
            int straddle = 0;
            for (int j = 0; j < kHeadW4 && j * kHeadThreads < h.w_total4; j++) straddle += h.piece_m[j] == -1;
            const int T = (e->fc[3].nout + 15) / 16;
            snprintf(line, sizeof line,
                     "head fwd=fused enc=%d grid=%dx%d stage=%s w4=%d late=%d straddle=%d fc0=%d:%d fc1=%d:%d fc2=%d:%d fc3=%d:%d lds=%zu\n",
                     h.n_enc, (batch + 15) / 16, (T + h.tiles_per_wg - 1) / h.tiles_per_wg, head_staging(h), h.w_total4,
                     (int)(h.w_total4 > kHeadEarly * kHeadThreads), straddle, h.fc_split[0].lg, h.fc_split[0].per, h.fc_split[1].lg,
                     h.fc_split[1].per, h.fc_split[2].lg, h.fc_split[2].per, h.fc_split[3].lg, h.fc_split[3].per, lds);
        } else {
            snprintf(line, sizeof line, "head fwd=layers why=%s\n", why);
        }
        s += line;
    }
    static const char* const kEpiName[] = {"raw_stats", "sigmse", "sigout", "raw"};   // S2Epi
    for (int l = 0; l < (int)e->dec.size(); l++) {
        const ConvLayer& L = e->dec[l];
        const int ci = L.cin, co = L.cout, kh = L.kh, kw = L.kw;
        char f[128], b[256];
        switch (choose_dec_fwd(e, L, l, batch, tr, ext)) {
            case DF_FUSED_LAST: {
                const LastPick p = choose_last(L, l > 0 && e->dec[l - 1].has_bn);
                snprintf(f, sizeof f, "last_fused<%d,%d,%d,%d> hb=%d vec4=%d bn=%d", ci, co, kh, kw, kLastHB, (int)p.vec4, (int)p.bn);
                break;
            }
            case DF_ROWS: {
                const RowsPick p = choose_rows_fwd(L);
                snprintf(f, sizeof f, "s2_fwd_rows<%d,%d,%d,%d>", ci, co, p.hb, 64 / p.lw);
                break;
            }
            case DF_S2: {
                const int epi = s2_fwd_epi(e, l, tr, ext);
                const S2FwdPick p = choose_s2_fwd(L, batch, epi);
                const char* fam = p.k == S2F_CS ? "s2_fwd_cs" : (p.k == S2F_QUAD ? "s2_fwd" : "s2_fwd2");
                snprintf(f, sizeof f, "%s<%d,%d,%d,%d,%d> epi=%s", fam, ci, co, kh, kw, p.tw, kEpiName[epi]);
                break;
            }
            case DF_CT_LDS: snprintf(f, sizeof f, "ct_fwd_lds<%d,%d>", kh, kw); break;
            case DF_IG: snprintf(f, sizeof f, "ig_fwd_s2"); break;
            case DF_UP: snprintf(f, sizeof f, "up"); break;
        }
        if (!tr) {
            snprintf(b, sizeof b, "-");
        } else {
            switch (choose_dec_bwd(e, L, l, batch, ext)) {
                case DB_FUSED_LAST: snprintf(b, sizeof b, "(fused)"); break;
                case DB_ROWS: {
                    const RowsPick p = choose_rows_bwd(L);
                    snprintf(b, sizeof b, "s2_bwd_rows<%d,%d,%d,3,3,%d,%d,%d>", ci, ci == 4 ? 4 : 2, co, p.hb, 64 / p.lw, p.d);
                    break;
                }
                case DB_S2: {
                    const S2BwdPick p = choose_s2_bwd(L);
                    if (p.k == S2B_DIRECT) snprintf(b, sizeof b, "s2_bwd2<%d,%d,%d,%d,%d>", ci, co, kh, kw, p.tw);
                    else if (p.k == S2B_SPLIT) snprintf(b, sizeof b, "s2_bwd_split<%d,%d,%d,%d,%d,%d>", ci, p.ct, co, kh, kw, p.tw);
                    else snprintf(b, sizeof b, "s2_bwd<%d,%d,%d,%d,%d>", ci, p.ct, co, kh, kw);
                    break;
                }
                case DB_CT_LDS: {   // what bwd_ct_lds launches: the kernel, its grid (groups, Cin / 16, parts) and the accumulator
                    CtBwdPlan p;
                    (void)ct_bwd_plan(e, batch, L, l, p);
                    snprintf(b, sizeof b, "ct_bwd_lds ctb_kernel=%s ctb_imgs=%d ctb_groups=%d ctb_parts=%d ctb_bands=%d ctb_hb=%d ctb_sharded=%d",
                             p.bands > 1 ? "band" : "lds", p.imgs, p.groups, p.parts, p.bands, p.hb, (int)(L.sh_w >= 0));
                    break;
                }
                case DB_IG: {
                    const IgBwdPlan p = ig_bwd_plan(L, batch);
                    snprintf(b, sizeof b, "ig_bwd_pair ig_ksplit=%d ig_tpw=%d ig_chunks=%d ig_per=%d ig_dgroup=%d ig_wn8=%d", p.ksplit,
                             p.tiles_per_wave, p.chunks, p.per, p.d_group, p.w_n8);
                    break;
                }
                case DB_GENERIC: snprintf(b, sizeof b, "wgrad+down"); break;
            }
        }
        snprintf(line, sizeof line, "dec%d fwd=%s bwd=%s\n", l, f, b);
        s += line;
    }
    {
        TailArgs t;
        size_t lds = 0;
        const char* why = "";
        bool tail_fused = false;
        if (!tr) {
            snprintf(line, sizeof line, "tail bwd=-\n");
        } else if ((tail_fused = tail_plan(e, a, t, lds, &why))) {
            const int rows = (batch + 15) / 16;
            snprintf(line, sizeof line, "tail bwd=fused rows=%d sums=%s g1=%d:%d g0=%d:%d gx=%d:%d w2=%d:%d w1=%d:%d w0=%d:%d lds=%zu\n", rows,
                     rows <= kStatShards ? "stored" : "added", t.sp_d[0].lg, t.sp_d[0].per, t.sp_d[1].lg, t.sp_d[1].per, t.sp_d[2].lg,
                     t.sp_d[2].per, t.sp_w[0].lg, t.sp_w[0].per, t.sp_w[1].lg, t.sp_w[1].per, t.sp_w[2].lg, t.sp_w[2].per, lds);
        } else {
            snprintf(line, sizeof line, "tail bwd=layers why=%s\n", why);
        }
        s += line;
        // the Linear backwards one by one (launch_backward): the GEMM pair and its input gradient's variant, or the generic kernels
        for (int i = 3; tr && !tail_fused && i >= 0; i--) {
            if (e->use_s2) snprintf(line, sizeof line, "fc%d bwd=pair burst=%d\n", i, (int)linear_bwd_burst(e, i));
            else snprintf(line, sizeof line, "fc%d bwd=generic\n", i);
            s += line;
        }
    }
    if (tr) {
        // the encoder's backward (launch_backward): layer 0's weight gradient rides in the optimiser launch of a cae_train_step
        // whose head was fused (enc_conv0_in_adam_ok), the inner layers take k_conv_bwd_pair
        const bool in_adam = head_fused && enc_conv0_fits_adam(e, a, e->enc[0]);
        snprintf(line, sizeof line, "enc conv0=%s inner=%s\n", in_adam ? "adam" : "own",
                 e->enc.size() < 2 ? "-" : (e->use_s2 && !a.syncing() ? "pair" : "layers"));
        s += line;
    }
    if ((int64_t)s.size() + 1 > out_bytes)
        return fail(CAE_ERR_ARG, "cae_debug_plan: the report needs %zu bytes, got %lld", s.size() + 1, (long long)out_bytes);
    memcpy(out, s.c_str(), s.size() + 1);
    return CAE_OK;
}

int cae_debug_wgrad_slabs(const cae_engine* e, int batch, char* out, int64_t out_bytes) {
    if (!e || !out || out_bytes < 1) return fail(CAE_ERR_ARG, "cae_debug_wgrad_slabs: bad argument");
    if (batch < 1 || batch > e->max_batch)
        return fail(CAE_ERR_ARG, "cae_debug_wgrad_slabs: batch %d outside 1 .. %d", batch, e->max_batch);
    const std::vector<WSlab> t = wgrad_slab_table(e, batch, e->variational, e->wslab_bytes);
    const WFold f = wgrad_fold_of(e, t);
    std::string s;
    char line[256];
    int64_t used = 0;
    for (size_t k = 0; k < t.size(); k++) {
        const WSlab& sl = t[k];
        snprintf(line, sizeof line, "dec%d writer=%s type=%s param=%lld values=%d partials=%d offset=%lld fold_wgs=%d fold_values=%d\n", sl.layer,
                 sl.writer, sl.f64 ? "f64" : "f32", (long long)e->dec[sl.layer].w_off, sl.nvals, sl.nparts, (long long)sl.off,
                 fold_wgs(sl.nvals, f.s[k].vshift), 1 << f.s[k].vshift);
        s += line;
        used = sl.off + (int64_t)sl.nparts * sl.nvals * (sl.f64 ? 8 : 4);
    }
    snprintf(line, sizeof line, "fold slabs=%d wgs=%d bytes=%lld capacity=%lld\n", f.nslab, f.nwg, (long long)used, (long long)e->wslab_bytes);
    s += line;
    if ((int64_t)s.size() + 1 > out_bytes)
        return fail(CAE_ERR_ARG, "cae_debug_wgrad_slabs: the report needs %zu bytes, got %lld", s.size() + 1, (long long)out_bytes);
    memcpy(out, s.c_str(), s.size() + 1);
    return CAE_OK;
}

}  // extern "C"
