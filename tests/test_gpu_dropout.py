"""Training with dropout ON against the float64 CPU oracle (oracle/ncf_oracle.py), on the MI355X.

Every other comparison with the oracle or the goldens runs at dropout 0, and every other test
with dropout > 0 holds two HIP forms of one step to each other.  Here the dropout stream is
restated on the host (tests/dropout_stream.py, plain numpy, from the device code's definition),
the kernels' keep-scales are held to it bit for bit, and the oracle runs the same step in
float64 with those masks: probabilities, loss, every dense gradient, the compact table gradients
and the parameters after Adam, at the tolerances of test_gpu_parity.test_train_vs_oracle:

    prob < 5e-6, loss < 5e-6, gradients rtol 2e-4 / atol 2e-6, parameters through
    tests/parity.py's sign-flip zones with atol 5e-6.

None of these is fitted to the GPU's output.  Their headroom was measured on the CPU with the
fp32 oracle against the float64 oracle on the same masks, per case (the figures stand beside
each case below): the fp32 oracle stays within a quarter of every tolerance.  ReLU kinks do not
decide a comparison: in the float64 oracle no tower pre-activation is closer to 0 than 4 x the
largest fp32-vs-float64 pre-activation difference measured for that case (``pre``, asserted).

A case may carry its own tower widths, temporal dim and MF table width (``hid``, ``tdim``,
``Dm``): the ``g_*`` cases run the per-layer path at the edges of the geometries the engine
accepts (D 16 to 256, head dim 8 and 64, M up to 64, widths 16 to 1024, one to four layers, the
two collections at different widths), and one test pins what lies just outside as refused.

Also here: the standalone MultiHeadAttention in training mode (attention.hip's LMAX 8 and 64
forms, masked and not) against O.mha(..., drop_mask=...) in float64.
"""
import numpy as np
import pytest
import torch

import _ncf_pkg
from oracle import ncf_oracle as O
from tests import dropout_stream as S
from tests.conftest import sub
from tests.parity import assert_params_close, zone_from_grads

pytestmark = pytest.mark.gpu
ncf = _ncf_pkg.load()
DEV = torch.device("cuda:0")

U, I, HID, TDIM, LR, WD = 400, 300, [256, 128, 64], 32, 1e-3, 1e-5
INIT_SEED = 21
TABLE_KEYS = {"mf_user": O.K_MF_U, "mf_item": O.K_MF_I, "mlp_user": O.K_MLP_U, "mlp_item": O.K_MLP_I}

# name: D, H, M, B, p, steps, kind, engine switches, data seed, and the CPU-side measurements
# of that case (fp32 oracle against the float64 oracle on the same masks, one host thread):
#   pre  = largest |fp32 - fp64| tower pre-activation (the kink margin is 4 x this);
#   the comment gives max |dprob|, |dloss|, the worst gradient element as a fraction of
#   2e-6 + 2e-4 |g|, and the smallest float64 |pre-activation| of the case.
# kind: "clock" = FusedTrainStep's default (deferred tables, device step clock: the step's seed
# is read from the clock); "host" = FusedTrainStep(deferred=False) (the seed drawn on the host
# each step); "reference" = model(kjt) -> BCE -> backward() -> torch.optim.Adam.step() (the
# first forward's seed drawn on the host, later ones from the clock the fused Adam attaches).
def _case(D, H, M, B, p, steps, kind, form, sw, data_seed, pre, **kw):
    return dict(D=D, H=H, M=M, B=B, p=p, steps=steps, kind=kind, form=form, sw=sw,
                data_seed=data_seed, pre=pre, **kw)


# form: what the step runs ("fused_small" / "fused_80": attention + tower in one launch per
# direction, small-batch or 80-row tiles; "block": the attention block and the tower's own
# launch; "unfused": projection GEMMs + attention.hip core + per-layer tower launches).
_UNFUSED = {"ATTN_BLOCK": False, "MLP_FUSED": False, "MLP_WGRAD": False}
_FP32_TOWER = {"BF16_MM": False}
CASES = {
    # the default step, 3 consecutive steps, each on its clock seed
    # CPU: |dprob| 1.59e-7, |dloss| 6.0e-8, gradient at 0.014 of its tolerance; nearest 8.35e-6
    "default": _case(64, 4, 5, 37, 0.2, 3, "clock", "fused_small", {}, 1696, 1.68e-6),
    # CPU: 1.38e-7, 9.0e-8, 0.010; nearest 8.16e-6
    "tiles80": _case(64, 4, 5, 37, 0.2, 2, "clock", "fused_80", {"SMALL_TILE_GROUPS": 0}, 739,
                     1.69e-6),
    # the three host-seeded forms share seeds and data.  CPU: 1.55e-7, 1.5e-8, 0.010; nearest 7.16e-6
    "unfused": _case(64, 4, 5, 37, 0.2, 2, "host", "unfused", _UNFUSED, 410, 1.75e-6),
    "block_stash": _case(64, 4, 5, 37, 0.2, 2, "host", "block",
                         {"FUSE_ATTN_TOWER": False, "ATTN_RC": False}, 410, 1.75e-6),
    "block_rc": _case(64, 4, 5, 37, 0.2, 2, "host", "block",
                      {"FUSE_ATTN_TOWER": False, "ATTN_RC": True}, 410, 1.75e-6),
    # the reference call pattern.  CPU: 1.37e-7, 2.2e-8, 0.011; nearest 6.74e-6
    "reference": _case(64, 4, 5, 37, 0.2, 2, "reference", "fused_small", {}, 142, 1.56e-6),
    # one head, M = 3.  CPU: 1.46e-7, 2.7e-8, 0.011; nearest 6.30e-6
    "h1_m3": _case(64, 1, 3, 50, 0.2, 2, "clock", "block", {}, 395, 1.42e-6),
    # M = 1: one key per row, whole attention weights dropped or doubled (p = 0.5)
    # CPU: 1.78e-7, 3.6e-8, 0.035; nearest 6.58e-6
    "m1": _case(64, 4, 1, 20, 0.5, 2, "clock", "block", {}, 44, 1.57e-6),
    # the C4 dims, padding rows inside a tile.  CPU: 1.71e-7, 5.5e-8, 0.015; nearest 1.22e-5
    "d128": _case(128, 8, 6, 19, 0.2, 2, "clock", "block", {}, 513, 2.01e-6),
    # bf16 tables under the fp32 tower, one step (tests/test_gpu_bf16.py), the reference on the
    # widened bf16 tables.  CPU: 1.74e-7, 1.44e-7, 0.014; nearest 1.33e-5
    "bf16_d64_p0": _case(64, 4, 5, 37, 0.0, 1, "host", "fused_small", _FP32_TOWER, 1, 1.52e-6,
                         table_dtype="bf16"),
    # CPU: 1.81e-7, 9.3e-8, 0.012; nearest 6.41e-6
    "bf16_d64_p02": _case(64, 4, 5, 37, 0.2, 1, "host", "fused_small", _FP32_TOWER, 1, 1.54e-6,
                          table_dtype="bf16"),
    # CPU: 1.15e-7, 1.3e-8, 0.020; nearest 4.94e-5
    "bf16_d128_p0": _case(128, 8, 6, 19, 0.0, 1, "host", "block", _FP32_TOWER, 2, 1.42e-6,
                          table_dtype="bf16"),
    # CPU: 1.15e-7, 7.2e-8, 0.016; nearest 7.56e-6
    "bf16_d128_p02": _case(128, 8, 6, 19, 0.2, 1, "host", "block", _FP32_TOWER, 4, 1.79e-6,
                           table_dtype="bf16"),
}

# The bf16 tower (engine.BF16_MM at its default: the tower's Linears on bf16 MFMA), one
# host-seeded step each; tests/test_gpu_bf16.py compares them with tests/bf16_tower.py's
# restatement and holds their CPU-side measurements (no ``pre``: the layer-by-layer comparison
# reads ReLU' from the step's own rows, and the end-to-end tolerances are measured flip noise).
# lw_*: the tower's own launch with a and dlin stored (weight gradients by wgrad.hip), and the
# same step with the weight gradients fused (*_fw).  e2e_*: the forms that keep everything in LDS.
_LW = {"FUSE_ATTN_TOWER": False, "MLP_WGRAD": False}
_LW_FW = {"FUSE_ATTN_TOWER": False, "MLP_WGRAD": True}


def _mm(D, H, M, B, p, form, sw, data_seed):
    return _case(D, H, M, B, p, 1, "host", form, sw, data_seed, None, table_dtype="bf16",
                 tower="bf16")


for _n, (_D, _H, _M, _B, _p) in {"d64_p0": (64, 4, 5, 37, 0.0), "d64_p02": (64, 4, 5, 37, 0.2),
                                  "d128_p0": (128, 8, 6, 19, 0.0), "d128_p02": (128, 8, 6, 19, 0.2),
                                  "b1_p02": (64, 4, 5, 1, 0.2)}.items():
    CASES["bf16mm_lw_" + _n] = _mm(_D, _H, _M, _B, _p, "block", _LW, 1)
    CASES["bf16mm_lw_" + _n + "_fw"] = _mm(_D, _H, _M, _B, _p, "block", _LW_FW, 1)
# (data seeds picked on the CPU: tests/test_gpu_bf16.py E2E)
CASES["bf16mm_e2e_small"] = _mm(64, 4, 5, 37, 0.2, "fused_small", {}, 3)
CASES["bf16mm_e2e_80"] = _mm(64, 4, 5, 37, 0.2, "fused_80", {"SMALL_TILE_GROUPS": 0}, 8)
CASES["bf16mm_e2e_d128"] = _mm(128, 8, 6, 19, 0.2, "block", {}, 5)


# The per-layer path at the edges of the geometries the engine accepts, under the default switches
# (form "generic": projection GEMMs or the attention block, attention.hip's core, one GEMM + row
# launch per tower layer, ncf_head_fwd/_bwd, the grouped weight gradients), 2 host-seeded steps each.
def _generic(D, H, M, B, p, hid, data_seed, pre, attn_block=False, **kw):
    return _case(D, H, M, B, p, 2, "host", "generic", {}, data_seed, pre, hid=hid,
                 attn_block=attn_block, **kw)


CASES.update({
    # every narrowest form (D = 16, head dim 8, W = 16), a one-layer tower
    # CPU: |dprob| 6.9e-8, |dloss| 3.7e-8, gradient at 0.0064 of its tolerance; nearest 1.51e-4
    "g_d16": _generic(16, 2, 2, 20, 0.2, [16], 2, 6.78e-8),
    # head dim 8 with M = 9: attention.hip's LMAX 64 core; W = 512: two float4 chunks per lane.
    # 10 of the data seeds 1..60 are admitted (the others leave a pre-activation within 4 x pre
    # of 0).  CPU: 1.09e-7, 5.8e-8, 0.024; nearest 1.47e-5
    "g_d32_m9": _generic(32, 4, 9, 6, 0.2, [512, 32], 50, 9.61e-7),
    # W = 1024 (four chunks), the head at 256 / 256, D = 256 gather, segment reduce and Adam.
    # Shrunk from B = 8: 24 rows x 1280 pre-activations, fp32 differences near 1e-5 (K = 1024 on
    # LayerNorm'd rows), and none of the data seeds 1..60 at B = 8 or 1..150 at B = 4 keeps every
    # pre-activation 4 x pre away from 0; at B = 3 seed 3 of 1..100 does (B = 2: seed 33 of 1..40).
    # CPU: 5.9e-8, 4.3e-8, 0.064; nearest 3.52e-5
    "g_d256": _generic(256, 4, 3, 3, 0.2, [1024, 256], 3, 5.10e-6),
    # M = 64 with B = 3, one head of 64, four layers, ncf_gemm_rows (64,128) / (128,128) / (128,64),
    # last width 16.  CPU: 8.2e-8, 6.8e-8, 0.012; nearest 2.84e-4
    "g_d64_m64": _generic(64, 1, 64, 3, 0.0, [128, 128, 64, 16], 4, 7.51e-7),
    # mf_embedding_dim 256 beside mlp_embedding_dim 32: the two collections at their own widths
    # CPU: 8.2e-8, 7.5e-8, 0.011; nearest 4.70e-5
    "g_split": _generic(32, 2, 5, 10, 0.2, [64, 32], 5, 7.27e-7, Dm=256),
    # the attention block feeding the per-layer tower.  CPU: 1.09e-7, 9.8e-8, 0.089; nearest 1.07e-5
    "g_block_tower": _generic(64, 8, 3, 12, 0.2, [128, 64], 5, 1.27e-6, attn_block=True),
})


def geo(c):
    """A case's tower widths, temporal dim and MF table width (0: the MLP tables' D); the
    defaults are what every case had before the generic ones."""
    return dict(hid=list(c.get("hid", HID)), tdim=c.get("tdim", TDIM), Dm=c.get("Dm", 0))


def make_model(D, H, M, p, hid=HID, tdim=TDIM, Dm=0):
    torch.manual_seed(INIT_SEED)
    return ncf.AdvancedNCF(U, I, 5, 24, Dm or D, D, tdim, list(hid), H, p, M - 1)


def make_batches(B, M, steps, data_seed):
    """Zipf-ish items (hot ids repeat: long segments), as test_train_vs_oracle."""
    g = torch.Generator().manual_seed(data_seed)
    out = []
    for _ in range(steps):
        u = torch.randint(0, U, (B,), generator=g).repeat_interleave(M)
        i = (torch.rand(B * M, generator=g) ** 3 * I).long().clamp_max(I - 1)
        t = torch.zeros(B, M)
        t[:, 0] = 1
        out.append((u, i, t.reshape(-1, 1)))
    return out


def host_seed(k):
    """The seed the next host-seeded step draws (torch.randint(0, 2**62, (1,)) on the default
    generator): seed the generator, draw once, seed it again, so that the step draws the same."""
    torch.manual_seed(k)
    s = int(torch.randint(0, 2 ** 62, (1,)).item())
    torch.manual_seed(k)
    return s


def torch_masks(seed, B, H, M, p, dtype=torch.float64, hid=HID):
    m = S.step_masks(seed, B, H, M, hid, p)
    return {"attn": torch.from_numpy(m["attn"]).to(dtype),
            "mlp": [torch.from_numpy(x).to(dtype) for x in m["mlp"]]}


def cast_state(sd, dtype):
    return {k: (v.detach().clone().to(dtype) if v.is_floating_point() else v.detach().clone())
            for k, v in sd.items()}


def tower_preacts(p, u, i, M, H, masks, hid=HID, tdim=TDIM):
    """The tower's pre-activations (the Linear outputs the ReLUs see) of the oracle's training
    forward, from the oracle's own pieces."""
    n = u.numel()
    g, b = p["mlp_norm.weight"], p["mlp_norm.bias"]
    xu = O.layer_norm(p[O.K_MLP_U][u], g, b).view(n // M, M, -1)
    xi = O.layer_norm(p[O.K_MLP_I][i], g, b).view(n // M, M, -1)
    att = O.mha(p, O.ATT, xu, xi, xi, H, masks["attn"]).reshape(n, -1)
    x = torch.cat([att, torch.zeros(n, tdim, dtype=att.dtype)], 1)
    out = []
    for l in range(len(hid)):
        z = O.linear(x, p[f"mlp.{4 * l}.weight"], p[f"mlp.{4 * l}.bias"])
        out.append(z)
        x = O.layer_norm(torch.relu(z), p[f"mlp.{4 * l + 2}.weight"], p[f"mlp.{4 * l + 2}.bias"])
        x = x * masks["mlp"][l]
    return out


def oracle_run(init, batches, seeds, H, M, p, dtype=torch.float64, linear=O.linear, hid=HID,
               tdim=TDIM):
    """The oracle's trajectory over ``batches`` with the masks of ``seeds`` (one per step), on
    one host thread (test_gpu_fullsize: torch's threaded CPU reductions do not fix their order).
    Per step: prob, loss, grads, the parameters before the step, the pre-activations.
    ``linear``: the tower's Linears (tests/bf16_tower.py restates the bf16 tower's)."""
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        ref = cast_state(init, dtype)
        opt = O.AdamState(lr=LR, weight_decay=WD)
        rec = []
        for (u, i, t), seed in zip(batches, seeds):
            masks = torch_masks(seed, u.numel() // M, H, M, p, dtype, hid)
            before = {k: v.clone() for k, v in ref.items()}
            with torch.no_grad():
                pre = tower_preacts(ref, u, i, M, H, masks, hid, tdim)
            prob, loss, grads = O.train_step(ref, opt, u, i, t.to(dtype), negative_samples=M - 1,
                                             num_heads=H, temporal_dim=tdim, n_layers=len(hid),
                                             dropout_masks=masks, linear=linear)
            rec.append(dict(prob=prob, loss=loss, grads=grads, before=before, pre=pre))
        return rec, ref
    finally:
        torch.set_num_threads(threads)


def case_seeds(name, steps):
    """The seeds a case's steps will use, worked out without a GPU (the CPU-side measurements
    are taken with them, tests/test_dropout_stream.py; the GPU tests assert them): host-seeded steps reseed the default generator with 1000 + s;
    under the clock the base seed is the draw that follows the model's construction."""
    c = CASES[name]
    if c["kind"] == "clock":
        make_model(c["D"], c["H"], c["M"], c["p"], **geo(c))
        base = int(torch.randint(0, 2 ** 62, (1,)).item())
        return [S.clock_seed(base, s) for s in range(steps)]
    if c["kind"] == "reference":
        # the first forward draws its seed on the host; the first optimizer.step() binds the
        # fused Adam, which draws the clock's base seed next, and later steps read the clock
        first = host_seed(1000)
        torch.randint(0, 2 ** 62, (1,))
        base = int(torch.randint(0, 2 ** 62, (1,)).item())
        return [first] + [S.clock_seed(base, s) for s in range(1, steps)]
    return [host_seed(1000 + s) for s in range(steps)]


def _set_switches(monkeypatch, switches):
    import ncf_amd.engine as E
    for k, v in switches.items():
        monkeypatch.setattr(E, k, v)


def _check_form(name, eng, D, H, M, B):
    """The predicate of the form that actually ran, as the A/B tests of test_gpu_parity assert
    theirs."""
    import ncf_amd.engine as E
    sw, form = CASES[name]["sw"], CASES[name]["form"]
    hid = geo(CASES[name])["hid"]
    fused_one_launch = eng.attn_tower_step(D, H, M, hid)
    if form == "generic":
        # under the default switches: the per-layer tower, behind the attention block or the
        # projection GEMMs + attention.hip core as the case states
        assert sw == {} and not eng.mlp_fused(D, hid) and not fused_one_launch
        assert eng.attn_block(D, H, M) == CASES[name]["attn_block"]
        assert eng.model.mlp_hidden_dims == hid and (eng.model.mf_embedding_dim != D) == bool(
            geo(CASES[name])["Dm"])
        return
    if form in ("fused_small", "fused_80"):
        assert fused_one_launch
        assert eng._tiles(B) == ("" if form == "fused_80" else "_small")
    elif form == "unfused":
        assert not eng.attn_block(D, H, M) and not eng.mlp_fused(D, hid)
        assert not eng.mlp_fused_wgrad() and not fused_one_launch
    else:
        assert form == "block"
        assert eng.attn_block(D, H, M) and eng.mlp_fused(D, hid) and not fused_one_launch
        assert eng.attn_rc(D, H, M) == sw.get("ATTN_RC", False)
    assert E.TOWER_SPLIT is False
    assert eng._tower_entry("ncf_mlp_fwd", True) == ("ncf_mlp_fwd" if "BF16_MM" in sw
                                                      else "ncf_mlp_fwd_bf16")


def _kjt(u, i):
    return ncf.KeyedJaggedTensor.from_lengths_sync(
        keys=["user_id", "product_id"], values=torch.cat([u, i]),
        lengths=torch.ones(2 * u.numel(), dtype=torch.long)).to(DEV)


def bf16_tables(sd):
    """The state with its four embedding tables rounded to bf16 and widened again."""
    out = dict(sd)
    for K in TABLE_KEYS.values():
        out[K] = sd[K].to(torch.bfloat16).float()
    return out


TOWER_KEYS = ("y", "mf_pred", "r", "a", "mean", "rstd", "dlin", "dy", "mlp_pred", "prob")


def gpu_run(name, monkeypatch, table_dtype=torch.float32, tower=False):
    """The case's steps on the GPU.  Returns (init state_dict on the CPU, batches, per-step
    records with the step's seed, final state_dict).  ``tower``: each record also carries the
    tower's tensors of the step's workspace (TOWER_KEYS; what the form that ran does not store
    is stale or uninitialised there) for tests/bf16_tower.py's layer-by-layer comparison."""
    from ncf_amd.trainer import FusedTrainStep
    c = CASES[name]
    D, H, M, B, p, steps, kind = (c[k] for k in ("D", "H", "M", "B", "p", "steps", "kind"))
    _set_switches(monkeypatch, c["sw"])
    m = make_model(D, H, M, p, **geo(c))
    init = {k: v.detach().clone() for k, v in m.state_dict().items()}
    m = m.to(DEV)
    eng = m.engine
    batches = make_batches(B, M, steps, c["data_seed"])
    step = opt = None
    if kind == "reference":
        opt = torch.optim.Adam(m.parameters(), lr=LR, weight_decay=WD)
        m.train()
    else:
        step = FusedTrainStep(m, lr=LR, weight_decay=WD, deferred=kind == "clock",
                              table_dtype=table_dtype)
        assert (step.clock is not None) == (kind == "clock")
        if table_dtype == torch.bfloat16:
            # the reference starts from what the step object holds: the tables rounded to bf16
            # (nearest even, as the CPU's cast) and widened; everything else untouched
            held = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
            want = bf16_tables(init)
            for k in init:
                assert torch.equal(held[k], want[k]), k
            assert all(v.dtype == torch.bfloat16 for v in step.tables_lp.values())
            init = held
    _check_form(name, eng, D, H, M, B)
    rec = []
    for s, (u, i, t) in enumerate(batches):
        uniq = {"user": torch.unique(u), "item": torch.unique(i)}
        # the step's seed: the device clock's when one is attached (FusedTrainStep's, or the one
        # the fused Adam behind torch.optim.Adam binds at its first step()), else the host's draw
        clock = step.clock if step is not None else eng.clock
        assert (clock is not None) == (kind == "clock" or (kind == "reference" and s > 0))
        seed = int(clock[1].item()) if clock is not None else host_seed(1000 + s)
        if kind == "reference":
            out = m(_kjt(u, i))
            loss = torch.nn.functional.binary_cross_entropy(out, t.to(DEV))
            opt.zero_grad()
            loss.backward()
            eng.materialize_table_grads()
            grads = {n: q.grad.detach().cpu().clone() for n, q in m.named_parameters()
                     if q.grad is not None}
            tab = {k: grads.pop(K)[uniq[k.split("_")[1]]] for k, K in TABLE_KEYS.items()}
            opt.step()
            prob, loss = out.detach().cpu(), loss.detach().cpu()
        else:
            w = step(u.to(DEV), i.to(DEV), t.to(DEV))
            torch.cuda.synchronize()
            nu = dict(zip(("user", "item"), w.num_unique.cpu().tolist()))
            assert torch.equal(w.uniq_u[:nu["user"]].cpu(), uniq["user"])
            assert torch.equal(w.uniq_i[:nu["item"]].cpu(), uniq["item"])
            prob, loss = w.prob.cpu().clone(), w.loss.cpu().clone()
            grads = {n: eng.grad_view(n).cpu().clone() for n in eng.dense_names}
            tab = {k: v[:nu[k.split("_")[1]]].cpu().clone() for k, v in w.G.items()}
        rec.append(dict(seed=seed, prob=prob, loss=loss, grads=grads, tab=tab, uniq=uniq))
        if tower:
            assert step is not None     # (the fused step hands its workspace back)
            tw = {k: getattr(w, k) for k in TOWER_KEYS}
            rec[-1]["tower"] = {k: [x.cpu().clone() for x in v] if isinstance(v, list)
                                else v.cpu().clone() for k, v in tw.items()}
            rec[-1]["tower"]["grads"] = grads
    if step is not None:
        step.sync()
    final = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    return init, batches, rec, final


def compare(name, init, batches, rec, final, params=True):
    """GPU records against the float64 oracle with the masks of each step's seed."""
    c = CASES[name]
    D, H, M, B, p = (c[k] for k in ("D", "H", "M", "B", "p"))
    hid, tdim = geo(c)["hid"], geo(c)["tdim"]
    seeds = [r["seed"] for r in rec]
    assert len(set(seeds)) == len(seeds)
    if p == 0:      # (every keep-scale is 1: the dropout-off leg of the bf16-table cases)
        assert all(float(x.min()) == 1.0 for x in S.step_masks(seeds[0], B, H, M, hid, p)["mlp"])
    ora, ref = oracle_run(init, batches, seeds, H, M, p, hid=hid, tdim=tdim)
    worst = dict(prob=0.0, loss=0.0, grad=0.0)
    zones = {}
    prev = None
    for s, (g, o, (u, i, t)) in enumerate(zip(rec, ora, batches)):
        masks = S.step_masks(g["seed"], B, H, M, hid, p)
        # not vacuous: the masks drop about p of their elements, and differ from step to step
        for x in ([masks["attn"]] + masks["mlp"]) if p > 0 else []:
            keep = float((x > 0).mean())
            assert abs(keep - (1 - p)) < 4 * (p * (1 - p) / x.size) ** 0.5, (s, x.shape, keep)
        if prev is not None and p > 0:
            assert not np.array_equal(prev["attn"], masks["attn"])
            assert all(not np.array_equal(a, b) for a, b in zip(prev["mlp"], masks["mlp"]))
        prev = masks
        # no ReLU kink decides a comparison (margin: 4 x the measured fp32-vs-fp64 difference)
        nearest = min(float(z.abs().min()) for z in o["pre"])
        assert nearest > 4 * c["pre"], (s, nearest, c["pre"])
        assert g["prob"].numel() == o["prob"].numel()
        gprob = g["prob"].double().reshape(o["prob"].shape)
        dp = (gprob - o["prob"]).abs().max().item()
        dl = abs(float(g["loss"]) - float(o["loss"]))
        worst["prob"], worst["loss"] = max(worst["prob"], dp), max(worst["loss"], dl)
        print(f"{name} step {s}: |dprob| {dp:.3g} |dloss| {dl:.3g}")
        assert dp < 5e-6, (s, dp)
        assert dl < 5e-6, (s, dl)
        dense = {k: v for k, v in o["grads"].items() if k not in TABLE_KEYS.values()}
        assert set(g["grads"]) == set(dense), set(g["grads"]) ^ set(dense)
        pairs = [(k, g["grads"][k], v) for k, v in dense.items()]
        pairs += [(k, g["tab"][k], o["grads"][K][g["uniq"][k.split("_")[1]]])
                  for k, K in TABLE_KEYS.items()]
        for k, got, want in pairs:
            got, want = got.double().numpy(), want.numpy()
            frac = float((np.abs(got - want) / (2e-6 + 2e-4 * np.abs(want))).max())
            worst["grad"] = max(worst["grad"], frac)
            np.testing.assert_allclose(got, want, rtol=2e-4, atol=2e-6, err_msg=f"{name} step {s} {k}")
        for k, v in o["grads"].items():
            zones.setdefault(k, []).append(zone_from_grads(v.numpy(), o["before"][k].numpy(), WD))
        if s == 0 and p > 0:
            # the masks of another seed are another function: the comparison can tell
            other = torch_masks(g["seed"] + 1, B, H, M, p, hid=hid)
            po = O.forward(cast_state(init, torch.float64), u, i, training=True,
                           negative_samples=M - 1, num_heads=H, temporal_dim=tdim,
                           n_layers=len(hid), dropout_masks=other)
            assert (gprob - po).abs().max().item() > 1e-3
    print(f"{name}: worst |dprob| {worst['prob']:.3g} |dloss| {worst['loss']:.3g} "
          f"gradient at {worst['grad']:.3g} of its tolerance")
    if params:
        for k, zs in zones.items():
            assert_params_close(k, final[k].numpy(), ref[k].numpy(), zs, LR, atol=5e-6)
    return worst


@pytest.mark.parametrize("name", [k for k in CASES if "table_dtype" not in CASES[k]])
def test_train_step_with_dropout_vs_float64_oracle(monkeypatch, name):
    init, batches, rec, final = gpu_run(name, monkeypatch)
    compare(name, init, batches, rec, final)
    # the seeds the CPU-side measurements were taken with (tests/test_dropout_stream.py)
    assert [r["seed"] for r in rec] == case_seeds(name, len(rec))


def test_geometries_outside_the_accepted_family_are_refused():
    """The edge of the family: D = 48, a tower width of 96 and head dim 4 are refused by name on
    the first training forward (argument checks, before the refusing entry point launches
    anything); a last width of 512 evaluates (ncf_head_fwd loops over any width) and is refused
    by ncf_head_bwd's size check when trained."""
    from ncf_amd.trainer import FusedTrainStep
    u, i, t = make_batches(6, 2, 1, 3)[0]

    def first_forward(D, H, hid):
        m = make_model(D, H, 2, 0.0, hid=hid).to(DEV)
        m.engine.forward(u.to(DEV), i.to(DEV), 2, True, 0.0, 0)

    for args, msg in (((48, 4, HID), r"unsupported embedding dim 48 \(16/32/64/128/256\)"),
                      ((64, 4, [96]), r"MLP width 96 unsupported \(powers of two 16\.\.1024\)"),
                      ((16, 4, [16]), r"head dim 4 unsupported \(8/16/32/64\)")):
        with pytest.raises((RuntimeError, ValueError), match=msg):
            first_forward(*args)
        torch.cuda.synchronize()
    hid = [64, 512]
    m = make_model(64, 4, 2, 0.0, hid=hid)
    init = {k: v.detach().clone() for k, v in m.state_dict().items()}
    m = m.to(DEV).eval()
    assert not m.engine.mlp_fused(64, hid)
    with torch.no_grad():
        prob = m(_kjt(u, i)).cpu().double().reshape(-1)
    want = O.forward(cast_state(init, torch.float64), u, i, training=False, negative_samples=0,
                     num_heads=4, temporal_dim=TDIM, n_layers=len(hid)).reshape(-1)
    assert (prob - want).abs().max().item() < 5e-6
    step = FusedTrainStep(m.train(), lr=LR, weight_decay=WD, deferred=False)
    with pytest.raises(ValueError, match=r"ncf_head_bwd: bad size \(width, dim <= 256\)"):
        step(u.to(DEV), i.to(DEV), t.to(DEV))
    torch.cuda.synchronize()


# ----------------------------------------------------------------------------- the stream itself
@pytest.mark.parametrize("p", [0.2, 0.25, 0.5])
@pytest.mark.parametrize("group,cols", [(1, 5), (1, 64), (1, 256), (16, 64), (16, 256)])
def test_dropout_rows_scales_equal_restatement(p, group, cols):
    """ncf_dropout_rows writes ncf_dropout_scale of index r * (cols / group) + c / group: bit
    for bit the host restatement's, over seeds with a zero / non-zero high word and rows whose
    index & 3 differs from row to row (cols = 5)."""
    from ncf_amd import _lib
    rows = 301
    per = cols // group
    x = torch.ones(rows, cols, device=DEV)
    for seed in (0, 12345, 2 ** 62 - 1, (0x1234ABCD << 32) | 0x9E3779B9):
        out = torch.empty(rows, cols, device=DEV)
        sc = torch.empty(rows, per, device=DEV)
        _lib.call("ncf_dropout_rows", x.data_ptr(), rows, cols, group, p, seed, out.data_ptr(),
                  sc.data_ptr(), _lib.stream_ptr(DEV))
        want = S.keep_scales(seed, rows * per, p).reshape(rows, per)
        assert np.array_equal(sc.cpu().numpy().view(np.uint32), want.view(np.uint32)), seed
        assert np.array_equal(out.cpu().numpy(), np.repeat(want, group, axis=1)), seed


# ----------------------------------------------------------------------------- standalone MHA
def _T(d):
    return {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in d.items()}


@pytest.mark.parametrize("tag,kind", [("mha5", None), ("mha50", None), ("mha5", "causal"),
                                      ("mha5", "padding")])
def test_mha_train_mode_vs_float64_oracle(f4, tag, kind):
    """ncf.MultiHeadAttention(D, H, dropout=0.3).train() on the F4 inputs (attention.hip's LMAX 8
    form for mha5, 64 for mha50), unmasked and with the causal / key-padding masks of
    test_mha_mask_vs_oracle: y, dq, dk, dv and every weight gradient against O.mha in float64
    with the restated keep-scales of the seed the call drew (ops.mha_forward), at that test's
    tolerances.  Two calls draw fresh masks; eval ignores dropout."""
    p = 0.3
    Bn, L, D, H = [int(x) for x in f4[f"{tag}/shape"]]
    w = _T(sub(f4, f"{tag}/w/"))
    mod = ncf.MultiHeadAttention(D, H, dropout=p)
    mod.load_state_dict(w)
    mod = mod.to(DEV).train()
    g = torch.Generator().manual_seed(3)
    mask = None
    if kind == "causal":
        mask = torch.tril(torch.ones(L, L, dtype=torch.bool))
    elif kind == "padding":
        lens = torch.randint(1, L + 1, (Bn,), generator=g)
        mask = (torch.arange(L)[None, :] < lens[:, None]).view(Bn, 1, 1, L)
    qkv = [torch.from_numpy(f4[f"{tag}/{n}"]) for n in "qkv"]
    gy = torch.from_numpy(f4[f"{tag}/gy"])
    xs = [t.to(DEV).requires_grad_(True) for t in qkv]
    seed = host_seed(77)
    y = mod(*xs, mask=None if mask is None else mask.to(DEV))
    y.backward(gy.to(DEV))
    keep = S.keep_scales(seed, Bn * H * L * L, p).reshape(Bn, H, L, L)
    frac = float((keep > 0).mean())
    assert abs(frac - (1 - p)) < 4 * (p * (1 - p) / keep.size) ** 0.5, frac
    ps = {f"a.{k}": v.double().requires_grad_(True) for k, v in w.items()}
    rs = [t.double().requires_grad_(True) for t in qkv]
    ry = O.mha(ps, "a.", *rs, H, drop_mask=torch.from_numpy(keep).double(), mask=mask)
    ry.backward(gy.double())
    print(f"mha {tag} {kind}: |dy| {(y.detach().cpu().double() - ry.detach()).abs().max().item():.3g}")
    torch.testing.assert_close(y.detach().cpu().double(), ry.detach(), atol=2e-5, rtol=1e-5)
    for a_, b_ in zip(xs, rs):
        torch.testing.assert_close(a_.grad.cpu().double(), b_.grad, atol=2e-5, rtol=1e-4)
    for n, q in mod.named_parameters():
        torch.testing.assert_close(q.grad.cpu().double(), ps[f"a.{n}"].grad, atol=5e-5, rtol=1e-4)
    # the masks of another seed: far outside the tolerance
    with torch.no_grad():
        other = O.mha({k: v.detach() for k, v in ps.items()}, "a.", *[t.detach() for t in rs], H,
                      drop_mask=torch.from_numpy(
                          S.keep_scales(seed + 1, Bn * H * L * L, p).reshape(Bn, H, L, L)).double(),
                      mask=mask)
        assert (y.detach().cpu().double() - other).abs().max().item() > 1e-3
        # fresh masks per call; eval ignores dropout
        margs = dict(mask=None if mask is None else mask.to(DEV))
        y2, y3 = mod(*xs, **margs), mod(*xs, **margs)
        assert not torch.equal(y2, y3)
        mod.eval()
        e1, e2 = mod(*xs, **margs), mod(*xs, **margs)
        assert torch.equal(e1, e2)
        plain = O.mha({k: v.detach() for k, v in ps.items()}, "a.", *[t.detach() for t in rs], H,
                      mask=mask)
        torch.testing.assert_close(e1.cpu().double(), plain, atol=2e-5, rtol=1e-5)
