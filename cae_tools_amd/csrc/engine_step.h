// engine_step.h - host only: one step of the ConvAE engine as a sequence of launches on e->stream.  The data-parallel gradient
// exchange, the forward and backward loops over the layers (one call per layer kind: engine_launch.h), the ops built from them
// and their hipGraph cache.
#pragma once

namespace {

// ---- data-parallel gradient exchange (cae_dp_train_step) -------------------------------------------
// Two buckets in the order backward completes them: [bucket_split, n_param) = Linear 3 and the decoder convolutions, ready
// as soon as Linear 3's backward has run, narrowed to fp32 and all-reduced on the second stream while the main stream
// still runs Linear 2..0 and the encoder backward; then [0, bucket_split) on the main stream once the first has finished
// (one communicator, one collective at a time, ordered on the device by the join event).
// Under SyncBN every collective (tables and buckets) stays on the main stream: the tables are on the critical path anyway.
StepTail narrow_tail(cae_engine* e, bool with_step_tail, int batch_inc) {
    StepTail t = step_tail_of(e, batch_inc, 1);
    if (!with_step_tail) {
        t.zero_extra = nullptr;
        t.zero_extra_n = 0;
        t.st = nullptr;
    }
    return t;
}

// k_adam over the parameter arena, from the fp32 gradients g32 (nullptr: from the fp64 accumulators), ending with the step tail
// tl; c0.on: c0.nw more workgroups take the first encoder layer's weight gradient (AdamConv0)
void adam_launch(cae_engine* e, const float* g32, const StepTail& tl, const AdamConv0& c0) {
    hipLaunchKernelGGL(k_adam, dim3(grid1(e->tab.n_param) + (c0.on ? c0.nw : 0)), dim3(256), 0, e->stream, (long long)e->tab.n_param,
                       e->params, g32, e->m, e->v, e->hp, (const StepState*)e->state(), e->shard_segs(), tl, 0, std::log(e->hp.beta1),
                       std::log(e->hp.beta2), c0);
}

int dp_allreduce_grads(cae_engine* e, int64_t lo, int64_t hi, hipStream_t on) {
    if (hi <= lo) return CAE_OK;
    NCCL_TRY(rccl().AllReduce(e->grads + lo, e->grads + lo, (size_t)(hi - lo), RcclApi::kFloat32, RcclApi::kSum, e->dp_comm, on));
    return CAE_OK;
}

// first bucket on the second stream (cae_dp_set_overlap)
bool dp_overlap(const cae_engine* e, const StepArgs& a) { return e->dp_overlap && !a.dp_sync; }

// Without the overlap (and without SyncBN) there is nothing to gain from two buckets: ONE narrowing launch and ONE all-reduce
// of the whole gradient arena after backward - one collective latency per step instead of two.
bool dp_single_collective(const cae_engine* e, const StepArgs& a) { return !dp_overlap(e, a) && !a.dp_sync; }

int dp_first_bucket(cae_engine* e, const StepArgs& a) {
    if (!a.dp || dp_single_collective(e, a)) return CAE_OK;
    const int64_t lo = e->bucket_split, hi = e->tab.n_param;
    const bool overlap = dp_overlap(e, a);
    hipStream_t on = overlap ? e->comm_stream : e->stream;
    if (overlap) {
        HIP_TRY(hipEventRecord(e->ev_fork, e->stream));
        HIP_TRY(hipStreamWaitEvent(e->comm_stream, e->ev_fork, 0));
    }
    {
        ProfScope _p(e, "dp_narrow_bucket0", 0, 12.0 * (hi - lo), on);
        hipLaunchKernelGGL(k_narrow_range, dim3(grid1(hi - lo)), dim3(256), 0, on, (long long)lo, (long long)hi, e->grads,
                           e->shard_segs(), narrow_tail(e, false, 0));
    }
    if (int rc = dp_allreduce_grads(e, lo, hi, on)) return rc;
    if (overlap) HIP_TRY(hipEventRecord(e->ev_join, e->comm_stream));
    return CAE_OK;
}

// after the last backward kernel: second bucket, join, Adam from the reduced fp32 gradients
int dp_finish_step(cae_engine* e, const StepArgs& a) {
    hipStream_t s = e->stream;
    const int64_t lo = 0, hi = dp_single_collective(e, a) ? e->tab.n_param : e->bucket_split;
    {
        ProfScope _p(e, "dp_narrow_bucket1", 0, 12.0 * (hi - lo));
        hipLaunchKernelGGL(k_narrow_range, dim3(grid1(hi - lo > 0 ? hi - lo : 1)), dim3(256), 0, s, (long long)lo, (long long)hi,
                           e->grads, e->shard_segs(), narrow_tail(e, true, a.inc()));
    }
    // the first bucket's all-reduce has to be over before the second is enqueued: one communicator runs one collective at a
    // time, and the join orders the two on the device (one fork + one join per step; the second bucket is last on the
    // critical path either way, so it runs on the main stream)
    if (dp_overlap(e, a)) HIP_TRY(hipStreamWaitEvent(s, e->ev_join, 0));
    if (int rc = dp_allreduce_grads(e, lo, hi, s)) return rc;
    ProfScope _p(e, "adam", 0, 28.0 * e->tab.n_param);
    adam_launch(e, e->grads, zeroed<StepTail>(), AdamConv0{});
    return CAE_OK;
}

int launch_forward(cae_engine* e, const StepArgs& a) {
    hipStream_t s = e->stream;
    const int B = a.batch;

    HeadArgs head;
    size_t head_lds = 0;
    const bool fused_head = a.part == 0 && head_plan(e, a, head, head_lds);
    if (fused_head) {
        head.x = a.x_direct ? a.x_direct : e->ds_x[a.which]; head.perm = a.x_direct ? nullptr : a.perm;
        head.use_cursor = a.x_direct ? 0 : 1; head.bump_adam = a.train ? 1 : 0;
        const int T = (e->fc[3].nout + 15) / 16;
        double bytes = 0;
        for (auto& L : e->enc) bytes += bytes_fwd(B, L);
        for (int i = 0; i < 4; i++) bytes += bytes_lin_fwd(B, e->fc[i]);
        head_lds_attr(k_head_fwd, head_lds);
        e->x_published = false;
        if (a.train) {
            // EVERY training forward clears the first encoder layer's BatchNorm table before anything adds to it: a fused
            // optimiser launch (AdamConv0) reads that table and therefore leaves it dirty, and which kind of step ran last
            // is not something a captured graph can know (the per-layer path below does the same with a fill launch)
            head.clear0 = e->bn_stats(e->enc[0].bn_index);
            head.clear0_n = kStatShards * e->enc[0].cout * 4;
            if (a.adam_follows) {
                head.xbatch = e->fptr(e->off_xbatch);
                e->x_published = true;
            }
        }
        ProfScope _p(e, a.train ? "head_fwd" : "head_eval", 0, bytes);
        hipLaunchKernelGGL(k_head_fwd, dim3((B + 15) / 16, (T + head.tiles_per_wg - 1) / head.tiles_per_wg), dim3(kHeadThreads),
                           head_lds, s, head);
    }
    if (!fused_head && a.train && a.part == 0)   // (see the fused launch above: every training forward clears this table first)
        HIP_TRY(hipMemsetAsync(e->bn_stats(e->enc[0].bn_index), 0, (size_t)kStatShards * e->enc[0].cout * 4 * sizeof(double), s));
    // ---- encoder convs
    for (int l = 0; !fused_head && a.part != 2 && l < (int)e->enc.size(); l++) {
        enc_conv_fwd(e, a, l);
        if (a.train)
            if (int rc = sync_bn_table(e, a, e->enc[l].bn_index)) return rc;
    }
    // ---- encoder_lin / decoder_lin
    if (!fused_head) {
        const ConvLayer& P = e->enc.back();
        const BnDesc bn_p = bn_of(e, P, a.train ? BN_BATCH : BN_RUNNING, (double)a.bn_batch * P.hout * P.wout, 1);
        const float* in = a.part == 2 ? a.z_in : e->fptr(P.act_off);
        const int fc_lo = a.part == 2 ? 2 : 0, fc_hi = a.part == 1 ? 2 : 4;
        for (int i = fc_lo; i < fc_hi; i++) {
            linear_fwd(e, a, i, in, P, bn_p);
            in = e->fptr(e->fc[i].act_off);
            if (i == 1 && e->variational && a.part != 1) {   // heads -> z (trunk_api.h; trunk_encode hands out the heads themselves)
                if (!e->hooks.reparam) return fail(CAE_ERR_STATE, "trunk engine without a reparameterisation hook");
                e->hooks.reparam(e->hooks.user, s, in, B, e->latent, a.train ? 1 : 0, e->fptr(e->off_vz));
                in = e->fptr(e->off_vz);
            }
        }
        if (a.part == 1) {   // the latent vector leaves the engine: (batch, latent) fp32, contiguous like the Linear's output
            HIP_TRY(hipMemcpyAsync(a.z_out, e->fptr(e->fc[1].act_off), sizeof(float) * (size_t)B * e->fc[1].nout, hipMemcpyDeviceToDevice, s));
            return CAE_OK;
        }
    }
    // ---- decoder conv-transposes
    for (int l = 0; l < (int)e->dec.size(); l++) {
        const DecFwd c = dec_fwd_operands(e, a, l);
        int rc = CAE_OK;
        switch (choose_dec_fwd(e, c.L, l, B, a.train, a.external_loss)) {
            case DF_FUSED_LAST: break;   // forward, loss and backward of this layer: one launch, in launch_backward
            case DF_ROWS: fwd_rows(e, a, c); break;
            case DF_S2: rc = fwd_s2(e, a, c); break;
            case DF_CT_LDS: fwd_ct_lds(e, a, c); break;
            case DF_IG: fwd_ig(e, a, c); break;
            case DF_UP: fwd_generic(e, a, c); break;
        }
        if (!rc && a.train && !c.last) rc = sync_bn_table(e, a, c.L.bn_index);   // the launch completed this layer's BatchNorm sums
        if (rc) return rc;
    }
    return CAE_OK;
}

int launch_backward(cae_engine* e, const StepArgs& a) {
    const int B = a.batch;
    // ---- decoder, last layer first
    for (int l = (int)e->dec.size() - 1; l >= 0; l--) {
        const ConvBwd c = conv_bwd_operands(e, a, e->dec, l);
        int rc = CAE_OK;
        switch (choose_dec_bwd(e, c.L, l, B, a.external_loss)) {
            case DB_FUSED_LAST: rc = bwd_last_fused(e, a, c); break;
            case DB_ROWS: bwd_rows(e, a, c); break;
            case DB_S2: rc = bwd_s2(e, a, c); break;
            case DB_CT_LDS: rc = bwd_ct_lds(e, a, c); break;
            case DB_IG: bwd_ig(e, a, c); break;
            case DB_GENERIC: bwd_generic(e, a, c); break;
        }
        if (!rc && c.prod.P) rc = sync_bn_table(e, a, c.prod.bn_index);   // the launch completed the producer's BatchNorm gradient sums
        if (rc) return rc;
    }
    // ---- Linear layers, last first
    {
        const ConvLayer& P = e->enc.back();
        TailArgs tail;
        size_t tail_lds = 0;
        const bool fused_tail = tail_plan(e, a, tail, tail_lds);
        for (int i = 3; i >= 0; i--) {
            if (i == 2)   // every decoder conv gradient and Linear 3's are complete: the first gradient bucket can leave
                if (int rc = dp_first_bucket(e, a)) return rc;
            if (fused_tail && i == 2) {
                tail_bwd(e, a, tail, tail_lds);
                break;
            }
            if (e->use_s2) {
                if (int rc = linear_bwd_pair(e, a, i, P)) return rc;
            } else {
                if (e->variational) return fail(CAE_ERR_STATE, "the trunk mode needs the specialised kernels (cae_set_kernel_mode)");
                linear_bwd_generic(e, a, i, P);
            }
            if (i == 0)
                if (int rc = sync_bn_table(e, a, P.bn_index)) return rc;
        }
    }
    // ---- encoder convs
    for (int l = (int)e->enc.size() - 1; l >= 0; l--) {
        const ConvBwd c = conv_bwd_operands(e, a, e->enc, l);
        if (l > 0 && e->use_s2 && !a.syncing()) {
            enc_conv_bwd_pair(e, a, c);
            continue;
        }
        memset(&e->c0_pending, 0, sizeof e->c0_pending);
        if (l == 0 && enc_conv0_in_adam_ok(e, a, c.L)) {
            enc_conv0_into_adam(e, a, c);
            continue;
        }
        enc_conv_bwd_generic(e, a, c);
        if (c.prod.P)
            if (int rc = sync_bn_table(e, a, c.prod.bn_index)) return rc;
    }
    return CAE_OK;
}

int launch_one(cae_engine* e, int op, const StepArgs& a);

int launch_op(cae_engine* e, int op, const StepArgs& a) {
    // the cursor lives on the device, so the same launch sequence repeated n times walks n batches:
    // n steps become one graph and the ~8.5 us the GPU idles between two graph replays is paid once
    for (int i = 0; i < a.nsteps; i++)
        if (int rc = launch_one(e, op, a)) return rc;
    return CAE_OK;
}

int launch_one(cae_engine* e, int op, const StepArgs& a) {
    hipStream_t s = e->stream;
    {   // while profiling: one EMPTY bracket per step = what an event pair itself adds to every bracketed launch
        ProfScope _cal(e, "event_pair", -1, 0.0);
    }
    if (op == OP_DP_TRAIN) {
        e->sync_pos = 0;
        if (a.batch > 0) {
            int rc = launch_forward(e, a);
            if (rc) return rc;
            rc = launch_backward(e, a);
            if (rc) return rc;
        } else {
            // a rank whose shard of a short last batch is empty: no kernels, but every collective of the step in order
            hipLaunchKernelGGL(k_bump_adam, dim3(1), dim3(1), 0, s, e->state());
            if (a.dp_sync)
                for (int bn : e->sync_order)
                    if (int rc = sync_bn_table(e, a, bn)) return rc;
            if (int rc = dp_first_bucket(e, a)) return rc;
        }
        if (a.dp_sync && e->sync_pos != e->sync_order.size())
            return fail(CAE_ERR_STATE, "SyncBN: %zu of %zu tables all-reduced", e->sync_pos, e->sync_order.size());
        if (int rc = dp_finish_step(e, a)) return rc;
    } else if (op == OP_TRAIN || op == OP_FWDBWD) {
        // the accumulators were zeroed by the previous step's last kernel (k_adam / k_acc_to_f32) or by
        // the caller's zero-filled workspace on the very first step
        StepArgs af = a;
        af.adam_follows = op == OP_TRAIN;
        memset(&e->c0_pending, 0, sizeof e->c0_pending);
        int rc = launch_forward(e, af);
        if (rc) return rc;
        rc = launch_backward(e, af);
        if (rc) return rc;
        if (op == OP_TRAIN) {
            ProfScope _p(e, "adam", 0, 32.0 * e->tab.n_param);
            AdamConv0 c0 = e->c0_pending;
            StepTail tl = step_tail_of(e, a.inc(), 1);
            if (c0.on) {
                // that layer's BatchNorm table (the first of the swept range) is read by this launch: the next step's
                // k_head_fwd clears it
                const long long skip = (long long)kStatShards * c0.C * 4;
                tl.zero_extra += skip;
                tl.zero_extra_n -= skip;
                c0.n_regular = grid1(e->tab.n_param);
            }
            adam_launch(e, nullptr, tl, c0);
        } else {
            hipLaunchKernelGGL(k_acc_to_f32, dim3(grid1(e->tab.n_param)), dim3(256), 0, s, (long long)e->tab.n_param, e->grads,
                               e->shard_segs(), step_tail_of(e, a.inc(), 1));
        }
    } else if (op == OP_EVAL) {
        int rc = launch_forward(e, a);
        if (rc) return rc;
        if (a.use_cursor) hipLaunchKernelGGL(k_advance, dim3(1), dim3(1), 0, s, e->state(), a.inc(), 1, 0);
    } else if (op == OP_ADAM) {
        // forward_backward already counted this optimiser step (its first kernel bumps adam_step)
        adam_launch(e, e->grads, zeroed<StepTail>(), AdamConv0{});
    }
    HIP_TRY(hipGetLastError());
    return CAE_OK;
}

// The learning rate lives in the step state on the device, where k_adam reads it: written here, by a one-thread launch in
// stream order, whenever the host's value has moved on (or the workspace is new).  Never inside a capture.
int push_lr(cae_engine* e) {
    if (!e->lr_stale || !e->ws) return CAE_OK;
    hipLaunchKernelGGL(k_set_lr, dim3(1), dim3(1), 0, e->stream, e->state(), e->hp.lr);
    HIP_TRY(hipGetLastError());
    e->lr_stale = false;
    return CAE_OK;
}

// run an op either directly or through a cached hipGraph
int run_op(cae_engine* e, int op, const StepArgs& a, bool cacheable) {
    if (int rc = push_lr(e)) return rc;
    // the legacy NULL stream cannot be captured: plain launches there
    if (!e->graph_mode || !cacheable || e->stream == nullptr || e->profiling)
        return e->capture_only ? CAE_OK : launch_op(e, op, a);
    // a SyncBN step and a per-rank-BatchNorm step of the same sizes are DIFFERENT launch sequences (table all-reduces,
    // bn_batch in every BatchNorm descriptor, the 1/world scale of the BatchNorm parameter gradients)
    auto key = std::make_tuple(op, a.which, a.batch, a.global_batch, (const void*)a.perm, a.nsteps, a.cursor_inc,
                               a.dp_sync ? 1 : 0, a.bn_batch, a.world);
    auto it = e->graphs.find(key);
    if (it == e->graphs.end()) {
        hipGraph_t graph = nullptr;
        HIP_TRY(hipStreamBeginCapture(e->stream, hipStreamCaptureModeThreadLocal));
        int rc = launch_op(e, op, a);
        hipError_t ce = hipStreamEndCapture(e->stream, &graph);
        if (rc) {
            if (graph) (void)hipGraphDestroy(graph);
            return rc;
        }
        if (ce != hipSuccess) return fail(CAE_ERR_HIP, "hipStreamEndCapture: %s", hipGetErrorString(ce));
        hipGraphExec_t exec = nullptr;
        hipError_t ie = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0);
        (void)hipGraphDestroy(graph);
        if (ie != hipSuccess) return fail(CAE_ERR_HIP, "hipGraphInstantiate: %s", hipGetErrorString(ie));
        it = e->graphs.emplace(key, exec).first;
        e->captures += 1;
    }
    if (e->capture_only) return CAE_OK;
    HIP_TRY(hipGraphLaunch(it->second, e->stream));
    return CAE_OK;
}

int check_ready(const cae_engine* e, int which, int batch, bool need_target) {
    if (!e) return fail(CAE_ERR_ARG, "null engine");
    if (!e->ws) return fail(CAE_ERR_STATE, "cae_bind has not been called");
    if (batch < 1 || batch > e->max_batch) return fail(CAE_ERR_ARG, "batch %d outside [1, %d]", batch, e->max_batch);
    if (which < 0 || which > 1) return fail(CAE_ERR_ARG, "dataset index %d is not 0 or 1", which);
    if (!e->ds_x[which]) return fail(CAE_ERR_STATE, "dataset %d has not been set", which);
    if (need_target && !e->ds_t[which]) return fail(CAE_ERR_STATE, "dataset %d has no target array", which);
    return CAE_OK;
}

}  // namespace
