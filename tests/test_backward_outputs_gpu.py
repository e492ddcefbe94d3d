"""The backward writes EVERY element of its outputs, whatever they held on entry.

`trace_surfels_backward` with `grads_out` / `accum_out` / `ray_grads_out` writes into caller-owned tensors; the sharded tracer hands it views
of one flat exchange buffer that it reuses from step to step.  Outside the prezero protocol (option grads_prezeroed = 0) nothing may survive
of what those tensors held: rows of Gaussians without a hit included, in every backward path.  Checked here with junk on entry (a large
value, NaN) against the same backward into all-zero tensors: bit for bit where the path sums in a fixed order (option deterministic), else
equal to rounding, and exactly zero wherever the reference run is zero.  End to end: two steps of a ShardedTracer with deferred weights and a
gradient exchange, where the second step misses Gaussians the first one hit (tests/xchg_accum_worker.py).
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from lidar_rt_amd import scenes

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

if torch.cuda.is_available():
    from tests.hip_util import DEV, DEFAULT_OPTS

GRADS = ("means", "scales", "rotations", "opacities", "shs")
# (options, bit-exact): the bucketed replay with each way of clearing the tensors (2 = default), the re-tracing backward asked for, the
# re-trace behind a hit record that overflowed, the re-trace behind a forward of the packet kernel.  The re-tracing paths add with float
# atomics in arrival order: equal to rounding only.
PATHS = {"bucketed-zip0": ({"zero_in_prep": 0, "deterministic": 1}, True), "bucketed-zip1": ({"zero_in_prep": 1, "deterministic": 1}, True),
         "bucketed-zip2": ({"zero_in_prep": 2, "deterministic": 1}, True), "bucketed-zip0-atomic": ({"zero_in_prep": 0}, False),
         "bwd_mode0": ({"bwd_mode": 0}, False), "record-overflow": ({"hit_cap": 8, "hit_cap_auto": 0}, False),
         "packet-forward": ({"fwd_mode": 0}, False)}


@pytest.fixture(scope="module")
def s10k():
    sc, o, d = scenes.s10k()
    return sc, o, d, scenes.upstream_grad(*o.shape[:2])


def _outputs(P, M, H, W, deferred, rays, fill):
    g = {"means": torch.empty((P, 3), device=DEV), "shs": torch.empty((P, M, 3), device=DEV), "opacities": torch.empty((P, 1), device=DEV),
         "scales": torch.empty((P, 2), device=DEV), "rotations": torch.empty((P, 4), device=DEV)}
    acc = torch.empty(P, device=DEV) if deferred else None
    rg = tuple(torch.empty((H, W, 3), device=DEV) for _ in range(2)) if rays else None
    for t in list(g.values()) + ([acc] if acc is not None else []) + (list(rg) if rg else []):
        t.fill_(fill)
    return g, acc, rg


@pytest.mark.parametrize("rays", [False, True], ids=["no-ray-grads", "ray-grads"])
@pytest.mark.parametrize("deferred", [False, True], ids=["accum-at-forward", "deferred-accum"])
@pytest.mark.parametrize("path", list(PATHS))
def test_backward_overwrites_junk_in_every_output(s10k, path, deferred, rays):
    from lidar_rt_amd.diff_lidar_tracer import _C
    sc, o, d, dL = s10k
    opts, exact = PATHS[path]
    H, W = o.shape[:2]; P, M = sc["shs"].shape[:2]
    st = _C.OptiXStateWrapper("")
    for k, v in {**DEFAULT_OPTS, **opts, "grads_prezeroed": 0, "deferred_accum": 1 if deferred else 0}.items():
        st.set_option(k, v)
    t = {k: torch.as_tensor(np.asarray(v, np.float32), device=DEV) for k, v in sc.items()}
    ro, rd = torch.as_tensor(o, device=DEV), torch.as_tensor(d, device=DEV)
    up = torch.as_tensor(dL, device=DEV)
    bg = torch.as_tensor(scenes.BG_DEFAULT, device=DEV)
    e = torch.empty(0, device=DEV)
    _C.build_from_gaussians(st, t["means"], t["scales"], t["rotations"], t["opacities"], 1.0)
    out, out_i, acc_fwd = _C.trace_surfels(st, True, ro, rd, e, bg, t["means"], t["shs"], 3, e, t["opacities"], t["scales"], 1.0,
                                          t["rotations"], e, e, e, e, False, False)
    torch.cuda.synchronize()
    st.check(DEV, wait=True)
    runs = {}
    fills = {"zero": 0.0, "large": 1.0e6, "nan": float("nan")}
    for name, fill in fills.items():
        g, acc, rg = _outputs(P, M, H, W, deferred, rays, fill)
        _C.trace_surfels_backward(st, ro, rd, e, bg, t["means"], t["shs"], 3, e, t["opacities"], t["scales"], 1.0, t["rotations"],
                                  e, e, e, e, False, False, out, out_i, up, grads_out=g, accum_out=acc, ray_grads_out=rg)
        torch.cuda.synchronize()
        res = {k: g[k].cpu().numpy() for k in GRADS}
        if acc is not None:
            res["accum"] = acc.cpu().numpy()
        if rg is not None:
            res["ray_o"], res["ray_d"] = rg[0].cpu().numpy(), rg[1].cpu().numpy()
        runs[name] = res
    ref = runs["zero"]
    weights = ref["accum"] if deferred else acc_fwd.cpu().numpy()
    assert (weights == 0).any() and (weights > 0).any(), "the scene must hold Gaussians with and without a hit"
    if deferred:
        assert not acc_fwd.cpu().numpy().any()
    for fill in ("large", "nan"):
        for k, v in runs[fill].items():
            r = ref[k]
            assert np.isfinite(v).all(), (path, fill, k, int((~np.isfinite(v)).sum()))
            np.testing.assert_array_equal(v[r == 0], 0.0, err_msg=f"{path} fill={fill} {k}: junk survived where the backward writes zero")
            if exact:
                np.testing.assert_array_equal(v, r, err_msg=f"{path} fill={fill} {k}")
            else:
                np.testing.assert_allclose(v, r, rtol=1e-4, atol=1e-6 * max(float(np.abs(r).max()), 1e-30), err_msg=f"{path} fill={fill} {k}")


@pytest.mark.parametrize("zero_in_prep", [0, 2])
def test_sharded_deferred_weights_of_a_second_step_with_another_hit_set(zero_in_prep):
    """Two steps of ShardedTracer(deferred_accum=True) with the collective code paths on (RCCL, one rank), exchanges dense / owner / auto;
    step 2 moves the sensor so that Gaussians hit in step 1 are missed.  Step 2's weights and their touched mask (accum > 0) must equal a
    fresh single-rank run of step 2."""
    worker = os.path.join(REPO, "tests", "xchg_accum_worker.py")
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT="29641", RANK="0", WORLD_SIZE="1", LOCAL_RANK="0", HSA_ENABLE_IPC_MODE_LEGACY="0",
               LRT_ZERO_IN_PREP=str(zero_in_prep))
    r = subprocess.run([sys.executable, worker], env=env, cwd=REPO, timeout=300, capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout or "")[-3000:] + (r.stderr or "")[-3000:]
    res = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert res["lost_in_step2"] > 0, res                       # step 2 misses Gaussians that step 1 hit
    for ex, v in res["exchanges"].items():
        assert v["last_exchange"] == ("sparse" if ex == "auto" else ex) or (ex == "auto" and v["last_exchange"] == "dense"), (ex, v)
        assert v["mask_mismatch"] == 0, (ex, v)
        assert v["rel_l2"] < 2e-6, (ex, v)
