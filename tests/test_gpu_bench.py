"""bench.py's plain run on the GPU at a tiny size, in process: the headline line's fields,
``--steps`` as the number of timed steps, and ``--dump-outputs`` (the last timed step's arrays,
identical from run to run: same arguments, same seeded inputs, no floating-point atomics on the
training path)."""
import contextlib
import io
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu

U, I, B, M, D = 3000, 700, 96, 5, 64
STEPS = 3
ARGS = ["--gpus", "1", "--steps", str(STEPS), "--warmup", "1", "--prime", "2", "--users", str(U),
        "--items", str(I), "--groups", str(B), "--batches", "4"]
NAMES = ("prob", "loss", "dense_params", "user_row_ids", "item_row_ids", "mf_user_rows",
         "mf_item_rows", "mlp_user_rows", "mlp_item_rows")


def _bench(extra):
    """bench.main() with ARGS + extra: (the one JSON line it printed, parsed)."""
    import bench
    buf = io.StringIO()
    with pytest.MonkeyPatch.context() as mp, contextlib.redirect_stdout(buf):
        mp.setattr(sys, "argv", [os.path.join(ROOT, "bench.py")] + ARGS + extra)
        for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
            mp.delenv(k, raising=False)
        bench.main()
    lines = [x for x in buf.getvalue().splitlines() if x.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """Two plain runs with the same arguments, each dumping its outputs:
    [(result line, {name: array}, files written)]."""
    out = []
    for k in range(2):
        d = tmp_path_factory.mktemp(f"dump{k}")
        rec = _bench(["--dump-outputs", str(d)])
        out.append((rec, {n: np.load(os.path.join(d, n + ".npy")) for n in NAMES},
                    sorted(os.listdir(d))))
    return out


def test_plain_line_is_the_headline(runs):
    rec = runs[0][0]
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "n_gpus"):
        assert k in rec, k
    assert rec["steps"] == STEPS and rec["warmup"] == 1 and rec["n_gpus"] == 1
    assert rec["unit"] == "samples/s" and rec["higher_is_better"] is True and rec["dtype"] == "fp32"
    assert rec["ms_per_step"] > 0
    # value = samples per second over the timed steps (both rounded: ms_per_step to 4 decimals,
    # value to 0.1)
    want = B * M / (rec["ms_per_step"] * 1e-3)
    assert abs(rec["value"] - want) <= want * (1e-4 / rec["ms_per_step"]) + 0.1
    # nothing but the headline ran
    for k in ("roofline", "infer", "dropin_train", "c4_train", "c5_scoring", "cpu_baseline",
              "kernel_ms_per_step", "c2_bf16_tables", "c2_b256", "c1_train"):
        assert k not in rec, k


def test_dump_holds_the_last_steps_outputs(runs):
    rec, a, files = runs[0]
    assert files == sorted(n + ".npy" for n in NAMES)
    N = B * M
    assert a["prob"].shape == (N,) and a["loss"].shape == (1,)
    # (U and I are below the sample size: every row, ids in order)
    assert np.array_equal(a["user_row_ids"], np.arange(U))
    assert np.array_equal(a["item_row_ids"], np.arange(I))
    for t, rows in (("mf_user", U), ("mlp_user", U), ("mf_item", I), ("mlp_item", I)):
        assert a[t + "_rows"].shape == (rows, D)
    for n, v in a.items():
        assert v.dtype == (np.float64 if n.endswith("_ids") else np.float32), n
        assert np.isfinite(v).all(), n
    assert sum(v.nbytes for v in a.values()) <= 64 * 2 ** 20
    assert (a["prob"] > 0).all() and (a["prob"] < 1).all()
    # prob and loss are of one step: the BCE of the dumped probabilities (target 1 on the first
    # row of every group of M) in float64.  The fp32 mean of N = 480 terms is within N eps
    # (480 x 6e-8 = 2.9e-5, worst case) of it, plus a few ulp per logarithm: 1e-4 relative
    p = a["prob"].astype(np.float64).reshape(B, M)
    bce = -(np.log(p[:, 0]).sum() + np.log1p(-p[:, 1:]).sum()) / N
    assert abs(float(a["loss"][0]) - bce) <= 1e-4 * bce
    assert abs(rec["final_loss"] - float(a["loss"][0])) <= 1e-6


def test_same_arguments_same_outputs(runs):
    (_, a, _), (_, b, _) = runs
    for n in NAMES:
        assert np.array_equal(a[n], b[n]), n
