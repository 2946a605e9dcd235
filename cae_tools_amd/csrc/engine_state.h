// engine_state.h - host only: the ConvAE engine's state (layers, arenas, workspace carve), the descriptor helpers its launch
// code builds kernel arguments from, the profile bracket and the arguments of a step.  Included by engine.hip alone, before
// engine_choose.h / engine_launch.h / engine_step.h (file map).
#pragma once

namespace {

constexpr float kBnEps = 1e-5f;      // nn.BatchNorm2d default (encoder.py:45, decoder.py:47)
constexpr float kBnMomentum = 0.1f;  // nn.BatchNorm2d default
constexpr int kLossSlots = 1 << 16;

int64_t align_up(int64_t v, int64_t a) { return (v + a - 1) / a * a; }

template <class T>
T zeroed() {   // kernel argument structs start from all zero bits
    T t;
    memset(&t, 0, sizeof t);
    return t;
}

struct ConvLayer {
    bool transposed;
    int cin, hin, win, cout, hout, wout, kh, kw, stride, opad;
    bool has_bn;
    int bn_index;  // index into the BN tables, -1 when has_bn is false
    int64_t w_off, b_off, gamma_off, beta_off;  // parameter arena (floats)
    int64_t rm_off, rv_off;                     // buffer arena (floats)
    int64_t act_off, grad_off;                  // workspace (bytes): raw output y / masked gradient g
    int sh_w = -1, sh_b = -1;                   // offsets in the sharded gradient table (-1: not sharded)
    int64_t out_elems() const { return (int64_t)cout * hout * wout; }
    int64_t in_elems() const { return (int64_t)cin * hin * win; }
};

struct FcLayer {
    int nin, nout;
    int64_t w_off, b_off;
    int64_t act_off, grad_off;  // output activation / gradient wrt pre-activation of the output
    bool relu;
};

}  // namespace

struct cae_engine {
    std::vector<ConvLayer> enc, dec;
    FcLayer fc[4];  // encoder_lin.0, encoder_lin.2, decoder_lin.0, decoder_lin.2
    int fc_size = 0, latent = 0, max_batch = 0;
    int in_c = 0, in_h = 0, in_w = 0, out_c = 0, out_h = 0, out_w = 0;
    TensorTable tab;
    int n_bn = 0;
    std::vector<int64_t> bn_stat_off;   // per BN: byte offset of its [C][4] double sums
    std::vector<int64_t> bn_saved_off;  // per BN: byte offset of its [C][2] float mean/invstd
    std::vector<int> bn_channels;
    int max_channels = 0;

    // workspace carve (byte offsets)
    int64_t off_state = 0, off_losses = 0, off_zero_begin = 0, off_gradacc = 0, off_zero_end = 0;
    int64_t off_glast = 0, off_sgacc = 0;
    ShardSegs segs{};                      // sharded gradient accumulators (thin stride-2 layers)
    int64_t ws_need = 0;

    // bound memory
    float *params = nullptr, *grads = nullptr, *m = nullptr, *v = nullptr, *bufs = nullptr;
    char* ws = nullptr;
    hipStream_t stream = nullptr;
    Hyper hp{1e-3, 0.9, 0.999, 1e-8, 1e-5};
    const float* ds_x[2] = {nullptr, nullptr};
    const float* ds_t[2] = {nullptr, nullptr};
    int64_t ds_n[2] = {0, 0};
    bool graph_mode = true;
    bool lr_stale = true;        // the device copy of hp.lr (StepState::lr) is behind the host's: push_lr() writes it
    long long captures = 0;      // graphs captured since creation (cae_graph_captures)
    bool capture_only = false;   // cae_set_capture_only: step calls capture + cache their graph and launch nothing
    bool use_s2 = true;  // specialised stride-2 kernels (cae_set_kernel_mode)
    // trunk of the 'var' model (trunk_api.h): fc[1] is the pair of heads [mu | logvar] (2 * latent outputs), z = reparam(heads)
    // feeds fc[2]; the loss lives outside, so the last decoder layer can hand out its raw output and take its gradient
    bool variational = false;
    int64_t off_vz = 0, off_vgz = 0, off_zlast = 0;
    cae_internal::TrunkHooks hooks{nullptr, nullptr, nullptr};
    bool gather_fwd = false;   // cae_set_kernel_mode bit 2: channel-rich decoder layers' forward on the gather kernel k_ig_fwd_s2
    int ctbwd_mask = 0;  // bit l: decoder layer l's backward runs the LDS-staged kernel (kernels_ctbwd.h) where eligible
    int ctbwd_auto = 0;  // ... the mask chosen at creation (the rule in cae_create): its layers have sharded accumulators
    int64_t off_xbatch = 0;     // the current batch's inputs, contiguous (written by k_head_fwd, read by k_adam's fused conv-0 weight gradient)
    bool x_published = false;   // this step's k_head_fwd wrote them
    AdamConv0 c0_pending{};     // filled by launch_backward when the conv-0 weight gradient is left to k_adam
    // weight-gradient partial slabs (engine_choose.h wgrad_slabs_on): a region outside the zeroed range, every slot is
    // overwritten by the step that reads it
    bool wgrad_atomics = false;   // cae_set_kernel_mode bit 3: weight-gradient partials by atomics, as before the slabs
    int64_t off_wslab = 0, wslab_bytes = 0;
    // profiling (cae_profile_begin/end): every launch bracketed by an event pair, plain launches
    bool profiling = false;
    struct ProfRec { const char* name; int layer; double bytes; hipEvent_t e0, e1; };
    std::vector<ProfRec> prof;
    // key: (op, which, batch, global_batch, perm, nsteps, cursor_inc, BatchNorm mode = (dp_sync, bn_batch, world)): everything
    // a captured launch sequence bakes in that is not engine-wide state (engine-wide changes call drop_graphs())
    std::map<std::tuple<int, int, int, int, const void*, int, int, int, int, int>, hipGraphExec_t> graphs;

    // data-parallel state (cae_dp_init): one RCCL communicator, a second stream for the gradient buckets, fork/join events
    int dp_world = 0, dp_rank = 0;
    RcclApi::comm_t dp_comm = nullptr;
    hipStream_t comm_stream = nullptr;
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    bool dp_graph_ok = true;            // RCCL calls captured inside the step graph (checked by cae_dp_init's self-test)
    bool dp_overlap = true;             // first gradient bucket on the second stream (cae_dp_set_overlap)
    std::vector<int> sync_order;        // BatchNorm tables in the order a SyncBN step all-reduces them
    size_t sync_pos = 0;
    int64_t bucket_split = 0;           // gradient buckets: [bucket_split, n_param) first (decoder), [0, bucket_split) last

    StepState* state() const { return reinterpret_cast<StepState*>(ws + off_state); }
    double* losses() const { return reinterpret_cast<double*>(ws + off_losses); }
    double* gradacc() const { return reinterpret_cast<double*>(ws + off_gradacc); }
    double* sgacc() const { return reinterpret_cast<double*>(ws + off_sgacc); }
    ShardSegs shard_segs() const {
        ShardSegs r = segs;
        r.base = sgacc();
        return r;
    }
    double* bn_stats(int j) const { return reinterpret_cast<double*>(ws + bn_stat_off[j]); }
    float* bn_saved(int j) const { return reinterpret_cast<float*>(ws + bn_saved_off[j]); }
    float* fptr(int64_t off) const { return reinterpret_cast<float*>(ws + off); }
    void drop_graphs() {
        for (auto& kv : graphs) (void)hipGraphExecDestroy(kv.second);
        graphs.clear();
    }
};

namespace {

// ---- descriptor helpers -----------------------------------------------------------------------

BnDesc bn_none() {
    BnDesc d = zeroed<BnDesc>();
    d.mode = BN_NONE;
    return d;
}

// BN descriptor of conv layer L's BatchNorm in `mode`; count = elements per channel
BnDesc bn_of(const cae_engine* e, const ConvLayer& L, int mode, double count, int update) {
    if (!L.has_bn) return bn_none();
    BnDesc d = zeroed<BnDesc>();
    d.mode = mode;
    d.C = L.cout;
    d.stats = e->bn_stats(L.bn_index);
    d.gamma = e->params + L.gamma_off;
    d.beta = e->params + L.beta_off;
    d.rmean = e->bufs + L.rm_off;
    d.rvar = e->bufs + L.rv_off;
    d.saved = e->bn_saved(L.bn_index);
    d.count = count;
    d.inv_count = count > 0.0 ? 1.0 / count : 0.0;
    d.unbias = count > 1.0 ? count / (count - 1.0) : 1.0;
    d.momentum = kBnMomentum;
    d.eps = kBnEps;
    d.update = update;
    return d;
}

Src src_plain(const float* p, int C, int H, int W) {
    Src s = zeroed<Src>();
    s.p = p;
    s.C = C;
    s.H = H;
    s.W = W;
    return s;
}

Epi epi_plain(float* out) {
    Epi e = zeroed<Epi>();
    e.kind = EPI_PLAIN;
    e.out = out;
    return e;
}

size_t lds_bytes(int c1, int c2) { return 4 * sizeof(double) + (size_t)(c1 + c2 + 1) * sizeof(float4); }

int grid1(int64_t n) { return (int)((n + 255) / 256); }
size_t gemm_lds(int channels) { return (4 * 256 + 256) * sizeof(float) + (size_t)(channels + 1) * sizeof(float4); }

// positions per block for k_wgrad: aim for ~2048 blocks in total, at least 256 positions each
int wgrad_ppb(int64_t positions, int64_t nweights) {
    int64_t target_blocks = 4096;
    int64_t nsplit = target_blocks / (nweights > 0 ? nweights : 1);
    if (nsplit < 1) nsplit = 1;
    int64_t ppb = (positions + nsplit - 1) / nsplit;
    if (ppb < 256) ppb = 256;
    ppb = align_up(ppb, 256);
    return (int)ppb;
}

enum Op { OP_TRAIN = 1, OP_FWDBWD = 2, OP_EVAL = 3, OP_ADAM = 4, OP_DP_TRAIN = 5 };

StepTail step_tail_of(cae_engine* e, int batch_inc, int slot_inc) {
    StepTail t = zeroed<StepTail>();
    t.zero_extra = reinterpret_cast<double*>(e->ws + e->off_zero_begin);
    t.zero_extra_n = (e->off_gradacc - e->off_zero_begin) / (long long)sizeof(double);
    t.acc_rw = e->gradacc();
    t.shard_rw = e->sgacc();
    t.st = e->state();
    t.batch_inc = batch_inc;
    t.slot_inc = slot_inc;
    return t;
}

// Brackets one launch with HIP events on the engine's stream while profiling is on.
// `bytes` = algorithmic bytes of the launch: every operand tensor read once, every result written once.
struct ProfScope {
    cae_engine* e;
    hipStream_t st;
    int idx = -1;
    ProfScope(cae_engine* e_, const char* name, int layer, double bytes, hipStream_t on = nullptr) : e(e_) {
        st = on ? on : e->stream;
        if (!e->profiling) return;
        cae_engine::ProfRec r{name, layer, bytes, nullptr, nullptr};
        if (hipEventCreate(&r.e0) != hipSuccess || hipEventCreate(&r.e1) != hipSuccess) return;
        (void)hipEventRecord(r.e0, st);
        e->prof.push_back(r);
        idx = (int)e->prof.size() - 1;
    }
    ~ProfScope() {
        if (idx >= 0) (void)hipEventRecord(e->prof[idx].e1, st);
    }
};

inline double f4(double n) { return 4.0 * n; }

// ---- the step, as a sequence of launches on e->stream -------------------------------------------

struct StepArgs {
    int which;
    const int32_t* perm;
    int batch;
    int global_batch;      // loss normalisation: batch summed over data-parallel ranks
    int bn_batch;          // samples behind the BatchNorm sums (local batch; global under SyncBN)
    bool train;            // train-mode forward (+ backward)
    bool use_cursor;       // samples come from the dataset through the cursor
    const float* x_direct; // score(): explicit input batch
    float* yhat;           // eval: sigmoid output destination (may be nullptr)
    bool want_loss;        // eval: accumulate MSE into the loss slot
    // SyncBN (cae_forward_backward_sync): after every launch that completes a BatchNorm sum table the
    // caller's function sums that table over the data-parallel ranks
    cae_allreduce_fn sync_fn = nullptr;
    void* sync_user = nullptr;
    int world = 1;
    bool ordered = false;  // trunk mode: every sync_fn call is checked against sync_order, as the dp_sync collectives are
    int nsteps = 1;        // consecutive steps of the same batch size in one captured graph
    // data-parallel step inside the library (cae_dp_train_step): gradient buckets all-reduced by RCCL on the second stream;
    // dp_sync additionally all-reduces every BatchNorm sum table in-stream (SyncBN) instead of calling sync_fn
    bool dp = false, dp_sync = false;
    int cursor_inc = -1;   // samples the cursor moves per step (-1: batch; the global batch under data parallelism)
    // module-level forward (cae_encode / cae_decode): 0 = the whole network, 1 = encoder only (x_direct -> z_out),
    // 2 = decoder only (z_in -> yhat); eval mode, per-layer launches
    bool external_loss = false;  // trunk mode: the last decoder layer writes its RAW output to off_zlast; its gradient arrives in off_glast
    bool adam_follows = false;   // OP_TRAIN on one device: k_adam is the next launch (it may take the first encoder layer's weight gradient)
    int part = 0;
    const float* z_in = nullptr;
    float* z_out = nullptr;
    bool syncing() const { return sync_fn != nullptr || dp_sync; }
    int inc() const { return cursor_inc >= 0 ? cursor_inc : batch; }
};

#define NCCL_TRY(expr)                                                                                            \
    do {                                                                                                          \
        int _r = (expr);                                                                                          \
        if (_r != 0) return fail(CAE_ERR_HIP, "%s failed: %s (%s:%d)", #expr, rccl().GetErrorString(_r), __FILE__, __LINE__); \
    } while (0)

int sync_bn_table(cae_engine* e, const StepArgs& a, int bn_index) {
    if (!a.syncing()) return CAE_OK;
    const int64_t n = (int64_t)kStatShards * e->bn_channels[bn_index] * 4;
    if (a.dp_sync) {
        // every rank must issue the same collectives in the same order: the order is a property of the model (sync_order),
        // and a step that deviates from it is an error here rather than a hang over there
        if (e->sync_pos >= e->sync_order.size() || e->sync_order[e->sync_pos] != bn_index)
            return fail(CAE_ERR_STATE, "SyncBN: table %d all-reduced out of order (position %zu)", bn_index, e->sync_pos);
        e->sync_pos++;
        NCCL_TRY(rccl().AllReduce(e->bn_stats(bn_index), e->bn_stats(bn_index), (size_t)n, RcclApi::kFloat64, RcclApi::kSum,
                                  e->dp_comm, e->stream));
        return CAE_OK;
    }
    if (a.ordered) {
        if (e->sync_pos >= e->sync_order.size() || e->sync_order[e->sync_pos] != bn_index)
            return fail(CAE_ERR_STATE, "SyncBN: table %d passed out of order (position %zu)", bn_index, e->sync_pos);
        e->sync_pos++;
    }
    return call_allreduce(ShardSync{a.sync_fn, a.sync_user}, "cae", e->bn_stats(bn_index), n);
}

// ---- facts of a layer that several launches share -------------------------------------------------------------------------

// (batch, small map, big map, kernel): a convolution's output and input, a transposed convolution's input and output
ConvGeom conv_geom(int B, const ConvLayer& L) {
    if (L.transposed) return ConvGeom{B, L.cin, L.hin, L.win, L.cout, L.hout, L.wout, L.kh, L.kw, L.stride};
    return ConvGeom{B, L.cout, L.hout, L.wout, L.cin, L.hin, L.win, L.kh, L.kw, L.stride};
}

// where conv layer L's backward adds its BatchNorm parameter gradients (all zero: L has no BatchNorm)
BnGradOut bn_grad_out(const cae_engine* e, const ConvLayer& L, const StepArgs& a) {
    BnGradOut bg = zeroed<BnGradOut>();
    if (!L.has_bn) return bg;
    bg.stats = e->bn_stats(L.bn_index); bg.C = L.cout; bg.scale = 1.0 / a.world;
    bg.gamma_acc = e->gradacc() + L.gamma_off; bg.beta_acc = e->gradacc() + L.beta_off;
    return bg;
}

// The producer of conv layer l of a chain: the layer whose BatchNorm'd output layer l reads.  Backward of layer l writes the
// gradient wrt the producer's raw output and adds to the producer's BatchNorm sum table, which is then the table to sync.
// The head of a chain has none (P == nullptr, no table, bn_prev none): the decoder's is fed by Linear 3, whose gradient
// buffer takes gin; the encoder's reads the data set and has no input gradient.
struct Producer {
    const ConvLayer* P = nullptr;
    float* gin = nullptr;           // gradient wrt the producer's raw output
    double* stats_in = nullptr;     // the producer's BatchNorm sum table
    const float* yprev = nullptr;   // the producer's raw output
    BnDesc bn_prev = bn_none();     // its BatchNorm from the statistics the forward pass saved
    int bn_index = -1;
};

Producer producer_of(const cae_engine* e, const std::vector<ConvLayer>& chain, int l, float* gin_head) {
    Producer p;
    p.gin = gin_head;
    if (l == 0) return p;
    const ConvLayer& P = chain[l - 1];
    p.P = &P; p.bn_index = P.bn_index;
    p.gin = e->fptr(P.grad_off); p.stats_in = e->bn_stats(P.bn_index);
    p.yprev = e->fptr(P.act_off); p.bn_prev = bn_of(e, P, BN_SAVED, 0, 0);
    return p;
}

Producer dec_producer(const cae_engine* e, int l) { return producer_of(e, e->dec, l, e->fptr(e->fc[3].grad_off)); }
Producer enc_producer(const cae_engine* e, int l) { return producer_of(e, e->enc, l, nullptr); }

// epilogue of a layer that feeds a BatchNorm: its raw output and, in a training step, the BatchNorm sums
Epi epi_raw_stats(const cae_engine* e, const ConvLayer& L, bool train) {
    Epi ep = epi_plain(e->fptr(L.act_off));
    if (!train) return ep;
    ep.kind = EPI_STATS; ep.stats = e->bn_stats(L.bn_index); ep.stats_C = L.cout;
    return ep;
}

// epilogue of a shape-generic input-gradient launch: masked by the producer's ReLU and summed into its table; plain at the head
Epi epi_gin(const Producer& p) {
    Epi ep = epi_plain(p.gin);
    if (!p.P) return ep;
    ep.kind = EPI_MASKSTATS; ep.stats = p.stats_in; ep.stats_C = p.P->cout; ep.yprev = p.yprev;
    return ep;
}

// ---- algorithmic bytes of a launch (ProfScope) ------------------------------------------------------------------------------
// forward of a conv layer: input and output once; with_target: a last layer that reads the target too
double bytes_fwd(int B, const ConvLayer& L, bool with_target = false) {
    return f4((double)B * (L.in_elems() + L.out_elems() * (with_target ? 2.0 : 1.0)));
}
// backward of a conv layer: gradient and raw output of the layer (the last layer: its gradient only), input activation and
// input gradient (head: no producer's output to mask by - or, for a weight-gradient launch, no input gradient)
double bytes_bwd(int B, const ConvLayer& L, bool last, bool head) {
    return f4((double)B * (L.out_elems() * (last ? 1.0 : 2.0) + L.in_elems() * (head ? 1.0 : 2.0)));
}
double bytes_lin_fwd(int B, const FcLayer& F) { return f4((double)B * (F.nin + F.nout) + (double)F.nin * F.nout); }
// backward of a Linear layer as a pair (k_gemm16_pair, k_tail_bwd): both GEMMs' operands and the fp64 weight accumulator
double bytes_lin_bwd_pair(int B, const FcLayer& F) {
    return f4((double)B * (3.0 * F.nin + 2.0 * F.nout) + (double)F.nin * F.nout) + 8.0 * F.nin * F.nout;
}

}  // namespace
