"""The four optimiser kernels against an fp64 Adam, element by element (tests/optim_ref.py holds the formulas, the value
regimes and the criterion; tests/test_optim_ref_cpu.py shows that the criterion sees a bias of 1.3e-5 of an update).

    k_adam      ConvAE (adam_step, OP_ADAM) and the VAE (apply_gradients -> trunk_adam_from)    Adam with L2 decay
    k_adam_l2   Linear                                                                          Adam with L2 decay
    k_adamw     UNET                                                                            AdamW

INJECTION.  params, exp_avg and exp_avg_sq are torch tensors the engines bind and never copy: a test writes (p, m, v) from
regimes(), hands over a gradient and reads the three back - no forward pass.  Every hyper set and step number of
optim_ref.CASES on every engine, a chain of eight steps, an arena of more than 2048 x 1024 parameters (k_adamw's second
grid-stride trip).  The step number: the UNET and Linear engines count on the host, set_step(t - 1) makes the next step number
t.  The ConvAE and its VAE trunk count on the device, and there forward_backward's first kernel counts the step that adam_step /
apply_gradients then takes: with no forward pass in front, the test loads t itself.

FUSED AGAINST SPLIT.  train_step against forward_backward + apply_gradients (ConvAE: + adam_step) from identical state with
non-zero moments, `strong` at t = 7: both narrow the same fp64 sum once, so the arenas are bit-identical - but for SPLIT_DIFFERS.

STALE GRAPHS.  cae_set_hyper drops the captured graphs when betas, eps or the decay change (they are kernel arguments).
"""
import functools

import numpy as np
import pytest
import torch

import optim_ref as R

pytestmark = pytest.mark.gpu

SEED = 41
N_SHARED = 20000          # the small engines' arenas are prefixes of one arena (regimes are index % 6): references computed once
STRONG = R.HYPERS["strong"][0]

# what beta1 = 0 does on each engine: "computed" - the step meets the criterion (exp_avg becomes the gradient itself).  None
# refuses the value; one that did would raise CaeError from set_hyper and stand here as "refused".
BETA1_ZERO = {"convae": "computed", "vae": "computed", "linear": "computed", "unet": "computed"}

# tensors that train_step and the split path do not give the same bits, by engine, and why.
#   ConvAE enc/encoder_cnn.0.weight: train_step leaves this gradient to k_adam's per-weight workgroups (AdamConv0: fp32 products,
#   one fp64 sum per weight), forward_backward accumulates it in the fp64 accumulators from the pair kernel's partial sums: a
#   different summation.  Held to the element-wise criterion with the split path's gradient instead; every later step then
#   starts both engines from the fused engine's values of it.
SPLIT_DIFFERS = {"convae": ("enc/encoder_cnn.0.weight",), "vae": (), "linear": (), "unet": ()}


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


class Rig:
    """one engine and the few calls that differ between the four"""

    def __init__(self, name, kind, eng, device_counter, extra=None):
        (self.name, self.kind, self.eng, self.device_counter, self.extra) = (name, kind, eng, device_counter, extra or {})
        self.n = eng.n_param
        tensors = getattr(eng, "tensors", None)
        if tensors is None:
            self.table = [(0, eng.nout * eng.nin, "linear.1.weight"), (eng.nout * eng.nin, eng.nout, "linear.1.bias")]
        else:
            self.table = sorted((off, numel, n) for n, (arena, off, numel, _) in tensors.items() if arena == 0)

    def name_of(self, i):
        last = "?"
        for (off, numel, n) in self.table:
            if off <= i < off + numel:
                return n
            if off + numel <= i:
                last = n
        return f"padding after {last}"

    def span(self, tensor):
        ((off, numel),) = [(o, k) for (o, k, n) in self.table if n == tensor]
        return slice(off, off + numel)

    def set_hyper(self, h, lr=None):
        self.eng.set_hyper(lr=h["lr"] if lr is None else lr, betas=h["betas"], eps=h["eps"], weight_decay=h["wd"], **self.extra)

    def write(self, p=None, m=None, v=None):
        self.eng.sync()
        for (dst, src) in ((self.eng.params, p), (self.eng.exp_avg, m), (self.eng.exp_avg_sq, v)):
            if src is not None:
                dst.copy_(_dev(src))
        torch.cuda.synchronize()

    def read(self):
        self.eng.sync()
        return tuple(a.cpu().numpy().copy() for a in (self.eng.params, self.eng.exp_avg, self.eng.exp_avg_sq))

    def completed(self, k):
        """k optimiser steps are complete (the next training step takes number k + 1)"""
        if self.name == "convae":
            self.eng.load_optimizer_state({}, k)
        else:
            self.eng.set_step(k)

    def inject(self, g, t=None):
        """the optimiser step from gradient g; t: its number (None: the engine's own count goes on)"""
        if t is not None:
            self.completed(t if self.device_counter else t - 1)     # (the module's header: who counts the step)
        if self.name == "convae":
            self.eng.grads.copy_(_dev(g))
            torch.cuda.synchronize()
            self.eng.adam_step()
        else:
            gd = _dev(g)
            torch.cuda.synchronize()
            self.eng.apply_gradients(gd)
        self.eng.sync()


# ---- the engines of the injection tests: the smallest that can be built ---------------------------------------------------------

def _conv_spec():
    from cae_tools_amd.models.model_sizer import create_model_spec
    return create_model_spec(input_size=(16, 16), input_channels=1, output_size=(28, 28), output_channels=1)


def _vae_spec():
    from cae_tools_amd.models.model_sizer import create_model_spec
    return create_model_spec(input_size=(12, 12), input_channels=1, output_size=(176, 176), output_channels=1)


def _unet_meta():
    from unet_helpers import UnetCase
    return UnetCase("u_k3s1_b2")


def _unet_extra(m):
    return dict(dropout_rate=m["dropout"], lambda_pearson=m["lambda_pearson"], seed=0)


def _make_rig(name):
    if name == "convae":
        from cae_tools_amd.engine import HipEngine
        return Rig(name, "adam", HipEngine(_conv_spec(), 16, 4, max_batch=2), True)
    if name == "vae":
        from cae_tools_amd.vae_engine import VaeEngine
        return Rig(name, "adam", VaeEngine(_vae_spec(), 12, 4, 1, device="cuda:0"), True, dict(seed=2))
    if name == "linear":
        from cae_tools_amd.linear_engine import LinearEngine
        rig = Rig(name, "adam", LinearEngine((1, 6, 7), (1, 3, 7), max_batch=2, device="cuda:0"), False)
        assert rig.n == 903
        return rig
    from cae_tools_amd.unet_engine import UnetEngine
    m = _unet_meta().meta
    return Rig(name, "adamw", UnetEngine(m["spec"], m["fc"], m["latent"], m["batch"], device="cuda:0"), False, _unet_extra(m))


ENGINES = ("convae", "vae", "linear", "unet")
_rigs = {}


@pytest.fixture(scope="module")
def rigs():
    def get(name):
        if name not in _rigs:
            _rigs[name] = _make_rig(name)
            print(f"\n[optimiser] {name}: n_param = {_rigs[name].n}")
            assert 64 <= _rigs[name].n <= N_SHARED
        return _rigs[name]
    yield get
    for rig in _rigs.values():
        rig.eng.close()
    _rigs.clear()


@functools.lru_cache(maxsize=None)
def _arena(n=N_SHARED, seed=SEED):
    return R.regimes(n, seed)


@functools.lru_cache(maxsize=None)
def _refs(kind, hyper, t):
    (_, p, g, m, v) = _arena()
    h = R.HYPERS[hyper][0]
    return R.torch_step(kind, "float32", p, g, m, v, t, **h), R.F64[kind](p, g, m, v, t, **h)


def _report(what, ratios):
    worst = {q: max(r for (_, qq), r in ratios.items() if qq == q) for q in R.QUANTITIES}
    zero = {q: ratios[("zero_state", q)] for q in R.QUANTITIES if ("zero_state", q) in ratios}
    print(f"\n[optimiser] {what}: worst ratio to the bound " + ", ".join(f"{q} {r:.3f}" for q, r in worst.items())
          + "; zero_state " + ", ".join(f"{q} {r:.3f}" for q, r in zero.items()))
    return worst


# ---- injection --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("hyper,t", R.CASES, ids=[f"{h}-t{t}" for h, t in R.CASES])
@pytest.mark.parametrize("engine", ENGINES)
def test_one_injected_step_against_fp64(rigs, engine, hyper, t):
    from cae_tools_amd._lib import CaeError
    rig = rigs(engine)
    n = rig.n
    (regime, p, g, m, v) = (a[:n] for a in _arena())
    try:
        rig.set_hyper(R.HYPERS[hyper][0])
    except CaeError as ex:
        assert hyper == "beta1_zero" and BETA1_ZERO[engine] == "refused" and "beta1" in str(ex), (engine, hyper, str(ex))
        return
    if hyper == "beta1_zero":
        assert BETA1_ZERO[engine] == "computed"
    rig.write(p, m, v)
    rig.inject(g, t)
    got = rig.read()
    (ref32, ref64) = (tuple(a[:n] for a in r) for r in _refs(rig.kind, hyper, t))
    for a in got:
        assert np.isfinite(a).all(), f"{engine}, {hyper}, t={t}: a non-finite value in the arenas"
    ratios = R.check_step(got, ref32, ref64, regime, p, f"{engine}, {hyper}, t={t}", rig.name_of)
    _report(f"{engine}, {hyper}, t={t}", ratios)
    # an optimiser that did nothing would not be here, but say so: the weights with a gradient moved (all but the odd one whose
    # new exp_avg cancels to less than an ulp of the weight)
    moved = got[0] != p
    assert moved[(g != 0) & (regime != R.REGIMES.index("eps_dominated"))].mean() > 0.99


@pytest.mark.parametrize("engine", ENGINES)
def test_a_chain_of_eight_injected_steps(rigs, engine):
    """eight steps at `strong`, a new gradient each, the state carried on the device.  Every step is held to the criterion with
    both references - torch in fp32 and the fp64 formula - restarted from the engine's own state before that step (so the bound
    is one step's rounding, never a trajectory's).  The UNET and Linear engines count the steps themselves."""
    rig = rigs(engine)
    n = rig.n
    (regime, p, _, m, v) = (a[:n] for a in _arena())
    rig.set_hyper(STRONG)
    rig.write(p, m, v)
    worst = {q: 0.0 for q in R.QUANTITIES}
    for t in range(1, 9):
        before = rig.read()
        g = R.regimes(n, SEED + t)[2]
        rig.inject(g, t if (rig.device_counter or t == 1) else None)
        got = rig.read()
        for a in got:
            assert np.isfinite(a).all(), f"{engine}, chain step {t}"
        args = (before[0], g, before[1], before[2], t)
        ratios = R.check_step(got, R.torch_step(rig.kind, "float32", *args, **STRONG), R.F64[rig.kind](*args, **STRONG), regime,
                              before[0], f"{engine}, strong, chain step {t}", rig.name_of)
        for (_, q), r in ratios.items():
            worst[q] = max(worst[q], r)
    print(f"\n[optimiser] {engine}, chain of 8 at strong: worst ratio " + ", ".join(f"{q} {r:.3f}" for q, r in worst.items()))
    if engine == "convae":
        assert rig.eng.adam_steps == 9      # load_optimizer_state(8) named the step being taken, adam_step counted it again
    elif rig.device_counter:
        assert rig.eng.steps == 9           # likewise set_step(8) + apply_gradients
    else:
        assert rig.eng.steps == 8


def test_the_second_grid_stride_trip_of_k_adamw():
    """adamw_blocks caps the grid at 2048 workgroups of 256 threads x 4 parameters: an arena above 2 097 152 parameters takes a
    second trip.  Injection only (max_batch 1: nothing steps through data), `default` at t = 2."""
    from cae_tools_amd.unet_engine import UnetEngine
    m = _unet_meta().meta
    eng = UnetEngine(m["spec"], 1092, m["latent"], 1, device="cuda:0")
    try:
        rig = Rig("unet", "adamw", eng, False, _unet_extra(m))
        n = rig.n
        print(f"\n[optimiser] unet, fc 1092: n_param = {n}")
        assert n > 2048 * 256 * 4
        (regime, p, g, m_, v) = R.regimes(n, SEED + 100)
        (hyper, t) = ("default", 2)
        h = R.HYPERS[hyper][0]
        rig.set_hyper(h)
        rig.write(p, m_, v)
        rig.inject(g, t)
        got = rig.read()
        ratios = R.check_step(got, R.torch_step("adamw", "float32", p, g, m_, v, t, **h), R.adamw_f64(p, g, m_, v, t, **h), regime, p,
                              f"unet (fc 1092), {hyper}, t={t}", rig.name_of)
        _report(f"unet (fc 1092, {n} parameters), {hyper}, t={t}", ratios)
        tail = slice(2048 * 256 * 4, n)
        assert ((got[0][tail] != p[tail]) | (g[tail] == 0)).any() and (got[2][tail] != v[tail]).any()
        # ... and the trip's elements alone
        R.check_step(tuple(a[tail] for a in got), tuple(a[tail] for a in R.torch_step("adamw", "float32", p, g, m_, v, t, **h)),
                     tuple(a[tail] for a in R.adamw_f64(p, g, m_, v, t, **h)), regime[tail], p[tail], "unet (fc 1092), second trip")
    finally:
        eng.close()


# ---- models with data: fused against split, stale graphs ---------------------------------------------------------------------

class _Model:
    """engine factory with weights, data and the `typical` moments of one geometry; step(eng) / split(eng) run one training
    step the fused way / as forward_backward + optimiser call, the latter returning the fp32 gradient (numpy)"""

    def __init__(self, name):
        self.name = name
        if name == "convae":
            from cae_tools_amd.models.decoder import Decoder
            from cae_tools_amd.models.encoder import Encoder
            self.spec = _conv_spec()
            torch.manual_seed(3)
            self.enc = Encoder(self.spec.get_input_layers(), encoded_space_dim=4, fc_size=16).state_dict()
            self.dec = Decoder(self.spec.get_output_layers(), encoded_space_dim=4, fc_size=16).state_dict()
            g = torch.Generator().manual_seed(4)
            self.batch = 3
            self.x = torch.rand((self.batch, 1, 16, 16), generator=g)
            self.t = torch.rand((self.batch, 1, 28, 28), generator=g)
        elif name == "vae":
            from test_vae_hip_parity import _setup
            self.batch = 2
            (self.spec, enc, dec, self.x, self.t) = _setup((12, 12), (176, 176), 12, 4, self.batch, seed=8)
            (self.enc, self.dec) = (enc.state_dict(), dec.state_dict())
        elif name == "linear":
            from test_linear_cpu import load
            (self.meta, z) = load("lin_2ch_b3")
            self.state = {k: z["init/" + k] for k in self.meta["keys"]}
            (self.x, self.t) = (torch.from_numpy(z["step0/x"]), torch.from_numpy(z["step0/t"]))
            self.batch = self.x.shape[0]
        else:
            self.case = _unet_meta()
            self.batch = self.case.meta["batch"]

    def rig(self, graph=True):
        name = self.name
        if name == "convae":
            from cae_tools_amd.engine import HipEngine
            eng = HipEngine(self.spec, 16, 4, max_batch=4, graph=graph)
            eng.load_state(self.enc, self.dec)
            eng.set_dataset(0, self.x.cuda(), self.t.cuda())
            rig = Rig(name, "adam", eng, True)
        elif name == "vae":
            from cae_tools_amd.vae_engine import VaeEngine
            eng = VaeEngine(self.spec, 12, 4, self.batch, device="cuda:0")
            eng.load_state(self.enc, self.dec)
            eng.set_dataset(0, self.x, self.t)
            rig = Rig(name, "adam", eng, True, dict(seed=2))
        elif name == "linear":
            from cae_tools_amd.linear_engine import LinearEngine
            eng = LinearEngine(self.meta["in_shape"], self.meta["out_shape"], max_batch=4, device="cuda:0")
            eng.load_state(self.state)
            eng.set_dataset(0, self.x, self.t)
            rig = Rig(name, "adam", eng, False)
        else:
            from cae_tools_amd.unet_engine import UnetEngine
            (c, m) = (self.case, self.case.meta)
            eng = UnetEngine(m["spec"], m["fc"], m["latent"], m["batch"], device="cuda:0")
            eng.load_state(c.state("init", "enc"), c.state("init", "dec"))
            (x, t, mk) = c.step_batch(0)
            eng.set_dataset(0, x.cuda(), t.cuda(), mk.cuda())
            rig = Rig(name, "adamw", eng, False, _unet_extra(m))
        (_, _, m_, v) = R.typical(rig.n, SEED + 7)
        rig.write(None, m_, v)
        return rig

    def step(self, rig):
        if self.name == "convae":
            rig.eng.train_step(0, None, 0, self.batch)
        else:
            rig.eng.train_step(0, None, 0, self.batch, slot=0)
        rig.eng.sync()

    def split(self, rig):
        eng = rig.eng
        if self.name == "convae":
            eng.forward_backward(0, None, 0, self.batch, self.batch)
            eng.sync()
            g = eng.grads.cpu().numpy().copy()
            eng.adam_step()
        else:
            gd = eng.forward_backward(0, None, 0, self.batch, slot=0)
            g = gd.cpu().numpy().copy()
            eng.apply_gradients(gd)
        eng.sync()
        return g


def _arenas(rig):
    rig.eng.sync()
    out = [("params", rig.eng.params), ("exp_avg", rig.eng.exp_avg), ("exp_avg_sq", rig.eng.exp_avg_sq)]
    if getattr(rig.eng, "buffers", None) is not None:
        out.append(("running statistics", rig.eng.buffers))
    return [(k, a.cpu().clone()) for k, a in out]


def _same_bits(a, b, what, rig=None, but=()):
    """the arenas of two engines, bit for bit - outside the element ranges `but` of the parameter-shaped ones"""
    for (k, u), (_, w) in zip(a, b):
        differ = u != w
        if k != "running statistics":
            for sl in but:
                differ[sl] = False
        if bool(differ.any()):
            i = int(torch.nonzero(differ)[0])
            where = f" ({rig.name_of(i)})" if rig is not None and k != "running statistics" else ""
            raise AssertionError(f"{what}: {k} differ in {int(differ.sum())} of {u.numel()} entries, the first at {i}{where}: "
                                 f"{float(u[i])!r} against {float(w[i])!r}")


@pytest.mark.parametrize("engine", ENGINES)
def test_train_step_equals_forward_backward_then_the_optimiser(engine):
    """step 1, 2: A fused, B split (two in a row: the accumulators and shard tables are left clear); step 3: A split after its
    fused steps, B fused after its split ones; step 4: both fused.  Bit-identical arenas after every step; a tensor of
    SPLIT_DIFFERS is held to the element-wise criterion with B's gradient and then copied from A to B."""
    model = _Model(engine)
    (a, b) = (model.rig(), model.rig())
    try:
        t0 = 7
        for rig in (a, b):
            rig.set_hyper(STRONG)
            rig.completed(t0 - 1)
        _same_bits(_arenas(a), _arenas(b), f"{engine}: two fresh engines")
        excepted = [a.span(k) for k in SPLIT_DIFFERS[engine]]
        order = (("fused", "split"), ("fused", "split"), ("split", "fused"), ("fused", "fused"))
        worst = 0.0
        for (k, (how_a, how_b)) in enumerate(order):
            t = t0 + k
            before = a.read()
            g = None
            for (rig, how) in ((a, how_a), (b, how_b)):
                if how == "fused":
                    model.step(rig)
                else:
                    g = model.split(rig)
            (sa, sb) = (_arenas(a), _arenas(b))
            for name, arena in sa:
                assert bool(torch.isfinite(arena).all()), f"{engine} step {t}: {name}"
            assert not torch.equal(sa[0][1], torch.from_numpy(before[0])), f"{engine} step {t}: the weights did not move"
            but = excepted if how_a != how_b else []
            _same_bits(sa, sb, f"{engine}, step {t} ({how_a} against {how_b})", a, but)
            for (tensor, sl) in zip(SPLIT_DIFFERS[engine], excepted):
                if how_a == how_b:
                    continue
                fused = a if how_a == "fused" else b
                got = tuple(x[sl] for x in fused.read())
                args = (before[0][sl], g[sl], before[1][sl], before[2][sl], t)
                ratios = R.check_step(got, R.torch_step(a.kind, "float32", *args, **STRONG), R.F64[a.kind](*args, **STRONG),
                                      np.zeros(sl.stop - sl.start, dtype=np.int8), before[0][sl],
                                      f"{engine}, strong, t={t}, {tensor} (fused, against the split path's gradient)")
                worst = max(worst, max(ratios.values()))
                # from here on both engines hold the fused engine's values of it
                other = b if fused is a else a
                for (dst, src) in ((other.eng.params, fused.eng.params), (other.eng.exp_avg, fused.eng.exp_avg),
                                   (other.eng.exp_avg_sq, fused.eng.exp_avg_sq)):
                    dst[sl].copy_(src[sl])
                torch.cuda.synchronize()
        if excepted:
            print(f"\n[optimiser] {engine}: {SPLIT_DIFFERS[engine]} fused against split, worst ratio to the bound {worst:.3f}")
        steps = (a.eng.adam_steps, b.eng.adam_steps) if engine == "convae" else (a.eng.steps, b.eng.steps)
        assert steps == (t0 - 1 + 4, t0 - 1 + 4), steps
        if engine != "linear":
            assert a.eng.num_batches_tracked == b.eng.num_batches_tracked == 4
    finally:
        a.eng.close()
        b.eng.close()


def test_a_hyper_change_drops_the_convae_graphs():
    """a graph-replayed train_step at `default`, then set_hyper with the `strong` betas, eps and decay (the rate unchanged: the
    rate is not a kernel argument): the next train_step from the same state differs from a replay under `default` and is, bit
    for bit, the step of a fresh engine that was given `strong` from the start (cae_set_hyper's drop_graphs())"""
    model = _Model("convae")
    (default, lr) = (R.HYPERS["default"][0], R.HYPERS["default"][0]["lr"])
    (a, fresh) = (model.rig(), model.rig())
    try:
        start = _arenas(a)

        def reload(rig):
            rig.eng.sync()
            for (_, src), dst in zip(start, (rig.eng.params, rig.eng.exp_avg, rig.eng.exp_avg_sq, rig.eng.buffers)):
                dst.copy_(src.cuda())
            torch.cuda.synchronize()
            rig.completed(6)

        outs = []
        a.set_hyper(default)
        for _ in range(2):                       # capture, then replay
            reload(a)
            model.step(a)
            outs.append(_arenas(a))
        assert a.eng.graph_captures() == 1 and a.eng.graph_count() == 1
        _same_bits(outs[0], outs[1], "capture against replay under default")
        a.set_hyper(STRONG, lr=lr)
        assert a.eng.graph_count() == 0
        reload(a)
        model.step(a)
        changed = _arenas(a)
        assert a.eng.graph_captures() == 2
        assert not torch.equal(changed[0][1], outs[1][0][1]) and not torch.equal(changed[2][1], outs[1][2][1])
        fresh.set_hyper(STRONG, lr=lr)
        reload(fresh)
        model.step(fresh)
        _same_bits(changed, _arenas(fresh), "after set_hyper against a fresh engine", a)
        # the running statistics and the loss do not depend on the optimiser's settings
        assert torch.equal(changed[3][1], outs[1][3][1])
    finally:
        a.eng.close()
        fresh.eng.close()


# ---- UNET: a LIN_BIG step (fp32 gradients in the fp64 slots, F32Ranges) and a step on the tile engine, one after the other ----

def test_unet_steps_on_either_side_of_lin_big():
    """choose_lin takes LIN_BIG up to batch 64 and the tile engine above (the partial-tile room is sized at min(max_batch, 64), so
    below 65 the choice does not depend on the batch: 64 and 65 are the two nearest sizes on either side).  A LIN_BIG step leaves
    fp32 gradients in the first half of fc0's and fc3's fp64 accumulator slots (fc_f32_dirty); the step after it, at the other
    size, must be the step of a fresh engine loaded with the state in between - in both orders."""
    from test_unet_shapes_gpu import _Model as ShapeModel
    from cae_tools_amd.unet_engine import UnetPlan
    model = ShapeModel("lin_k1296", rows=65)
    plan = UnetPlan(model.spec, model.fc, model.latent, 65)
    try:
        kinds = {b: plan.kernel_plan(b, True)["fc0"]["fwd"] for b in (64, 65)}
        assert kinds == {64: "lin_big", 65: "tile"}, kinds
        assert plan.n_param % 4 == 0 and all(off % 4 == 0 for (_, off, _, _) in plan.tensors.values())
    finally:
        plan.close()
    (_, _, m_, v) = R.typical(plan.n_param, SEED + 9)

    def engine():
        rig = Rig("unet", "adamw", model.engine(65), False, dict(dropout_rate=0.1, seed=4))
        rig.set_hyper(STRONG)
        return rig

    for (first, second) in ((64, 65), (65, 64)):
        a = engine()
        b = engine()
        try:
            a.write(None, m_, v)
            a.completed(6)
            a.eng.train_step(0, None, 0, first, slot=0)
            between = _arenas(a)
            a.eng.train_step(0, None, 0, second, slot=1)
            # (the arenas as they are: the padding between the tensors takes AdamW's step with the rest, load_state would skip it)
            b.write(*(x.numpy() for _, x in between[:3]))
            b.eng.buffers.copy_(between[3][1].cuda())
            torch.cuda.synchronize()
            b.completed(7)
            _same_bits(between, _arenas(b), f"{first} then {second}: the state in between, loaded")
            b.eng.train_step(0, None, 0, second, slot=1)
            (sa, sb) = (_arenas(a), _arenas(b))
            assert all(bool(torch.isfinite(x).all()) for _, x in sa)
            _same_bits(sa, sb, f"a step at batch {second} after one at {first}, against a fresh engine", a)
            assert a.eng.read_losses(1, 1) == b.eng.read_losses(1, 1)
        finally:
            a.eng.close()
            b.eng.close()
