"""Every Gaussian's gradient row (`d_means`, `d_scales`, `d_rotations`, `d_opacities`, `d_shs`) and hit weight (`accum`) of every backward path
against the float64 oracle, row by row: the gate of tests/row_gate.py (every row within 1e-3 of its own size plus a floor taken from the float32
oracle's worst row; untouched rows and inactive SH coefficients exact zeros; at least 70 % of the touched rows sensitive).

A case runs build -> training forward -> (the host looks at the outputs and the hit record and masks the event rays: at most 2 %) -> backward
with the masked upstream gradient, through the calls the Tracer makes (`_C.trace_surfels`, `_C.trace_surfels_backward`) into tensors of the
test's own: filled with NaN on entry, or all-zero under option grads_prezeroed.  The speculative path repeats the step without the host in
between (the second backward is enqueued behind its forward) and then checks that the second forward had no event ray outside the mask.
The composited sequences come from the path's own hit record; the paths that keep no complete one (packet forward, an 8-hit record) are
compared through the record of the default forward of the same scene, and through their own outputs.  Prints ROWGRAD|case|path|tensor|c|worst|
sensitive per tensor and ROWCASE|case|path|masked rays|float32 oracle's event rays per run."""
import numpy as np
import pytest
import torch

from lidar_rt_amd import scenes
from tests import row_gate
from tests.row_gate import BG3, GRADS, MAX_MASKED, Reference, SCENES, scene
from tests.test_ray_grads_gpu import PATHS

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from tests.event_gate import hip_sequences
    from tests.hip_util import DEV, DEFAULT_OPTS

PATH_IDS = [p[3] for p in PATHS]
_REFS, _DEFAULT_SEQS = {}, {}


@pytest.fixture(scope="module")
def refs():
    """Both oracles of a case, computed once per module: refs(key, make) -> Reference."""
    def get(key, make):
        if key not in _REFS:
            _REFS[key] = make()
        return _REFS[key]
    yield get
    _REFS.clear(); _DEFAULT_SEQS.clear()


def _own_record(opts):
    return opts.get("fwd_mode", 2) == 2 and "hit_cap" not in opts


def _record(st, ref):
    """The composited sequences of the last forward; a ray that filled its record counts as an event ray (no sequence equals [-1])."""
    seqs, full, _ = hip_sequences(st, ref.HW)
    return [np.array([-1]) if full[r] else seqs[r] for r in range(ref.HW)]


def _step(st, ref, t, opts, deferred, rays, prezeroed, dL_of, sync):
    """One build + forward + backward.  dL_of(out, seqs) -> upstream gradient (called after a synchronisation when `sync`, else with (None, None))."""
    from lidar_rt_amd.diff_lidar_tracer import _C
    H, W, P, M = ref.H, ref.W, ref.P, ref.sc["shs"].shape[1]
    e = torch.empty(0, device=DEV)
    bg = torch.as_tensor(np.asarray(ref.bg, np.float32), device=DEV)
    _C.build_from_gaussians(st, t["means"], t["scales"], t["rotations"], t["opacities"], ref.mod)
    out, out_i, acc_fwd = _C.trace_surfels(st, True, t["o"], t["d"], e, bg, t["means"], t["shs"], ref.deg, e, t["opacities"], t["scales"], ref.mod,
                                          t["rotations"], e, e, e, e, False, False)
    seqs = None
    if sync:
        torch.cuda.synchronize()
        st.check(DEV, wait=True)
        seqs = _record(st, ref) if _own_record(opts) else None
        dL = dL_of(out.cpu().numpy(), seqs)
    else:
        dL = dL_of(None, None)
    fill = 0.0 if prezeroed else float("nan")
    g = {"means": (P, 3), "shs": (P, M, 3), "opacities": (P, 1), "scales": (P, 2), "rotations": (P, 4)}
    g = {k: torch.full(shp, fill, device=DEV) for k, shp in g.items()}
    acc = torch.full((P,), fill, device=DEV) if deferred else None
    rg = tuple(torch.full((H, W, 3), float("nan"), device=DEV) for _ in range(2)) if rays else None
    _C.trace_surfels_backward(st, t["o"], t["d"], e, bg, t["means"], t["shs"], ref.deg, e, t["opacities"], t["scales"], ref.mod, t["rotations"],
                              e, e, e, e, False, False, out, out_i, torch.as_tensor(np.asarray(dL, np.float32), device=DEV),
                              grads_out=g, accum_out=acc, ray_grads_out=rg)
    torch.cuda.synchronize()
    st.check(DEV, wait=True)
    if not sync:
        seqs = _record(st, ref) if _own_record(opts) else None
    res = {k: g[k].cpu().numpy() for k in GRADS}
    res["accum"] = (acc if deferred else acc_fwd).cpu().numpy().reshape(-1, 1)
    if rays:
        assert all(np.isfinite(r.cpu().numpy()).all() for r in rg)
    return res, out.cpu().numpy(), seqs


def _default_seqs(key, ref, t):
    """The composited sequences of the default forward of this case (for the paths without a complete record of their own)."""
    if key not in _DEFAULT_SEQS:
        from lidar_rt_amd.diff_lidar_tracer import _C
        st = _C.OptiXStateWrapper("")
        for k, v in {**DEFAULT_OPTS, "hit_cap_auto": 1, "grads_prezeroed": 0, "deferred_accum": 0, "deterministic": 0}.items():
            st.set_option(k, v)
        _DEFAULT_SEQS[key] = _step(st, ref, t, {}, False, False, False, lambda out, seqs: ref.dL, True)[2]
    return _DEFAULT_SEQS[key]


def run_case(key, ref, path, rays=False, prezeroed=False, report=None):
    from lidar_rt_amd.diff_lidar_tracer import _C
    opts, kw, steps, what = path
    deferred = bool(kw.get("deferred_accum") or kw.get("deterministic"))
    t = {k: torch.as_tensor(np.asarray(v, np.float32), device=DEV) for k, v in ref.sc.items()}
    t["o"] = torch.as_tensor(np.asarray(ref.o, np.float32), device=DEV); t["d"] = torch.as_tensor(np.asarray(ref.d, np.float32), device=DEV)
    fallback = None if _own_record(opts) else _default_seqs(key, ref, t)
    st = _C.OptiXStateWrapper("")
    for k, v in {**DEFAULT_OPTS, "hit_cap_auto": 1, **opts, "grads_prezeroed": 1 if prezeroed else 0, "deferred_accum": 1 if deferred else 0,
                 "deterministic": 1 if kw.get("deterministic") else 0}.items():
        st.set_option(k, v)
    state = {}

    def events(out, seqs):
        return ref.event_rays(out, seqs if seqs is not None else fallback)

    def first(out, seqs):
        state["mask"] = events(out, seqs) | ref.f32_events
        state["seqs"] = seqs if seqs is not None else fallback
        return ref.masked_dL(state["mask"])

    res, out, seqs = _step(st, ref, t, opts, deferred, rays, prezeroed, first, True)
    mask = state["mask"]
    for _ in range(steps - 1):                          # the speculative backward: no host in between, the same mask, checked afterwards
        res, out, seqs = _step(st, ref, t, opts, deferred, rays, prezeroed, lambda o_, s_: ref.masked_dL(mask), False)
        late = events(out, seqs) & ~mask
        assert not late.any(), (key, what, "event rays of the second forward outside the mask", np.nonzero(late)[0][:8])
        state["seqs"] = seqs if seqs is not None else fallback
    tag = what + (" +rays" if rays else "") + (" +prezeroed" if prezeroed else "")
    line = f"ROWCASE|{key}|{tag}|{int(mask.sum())} of {ref.HW} rays masked|{int(ref.f32_events.sum())} float32-oracle event rays"
    print(line)
    if report is not None:
        report.append(line)
    assert mask.mean() <= MAX_MASKED, (key, tag, int(mask.sum()))
    assert not (ref.output_edges(out) & ~mask).any()    # every unmasked ray within 1e-4 of the float64 output
    bw = ref.backward(mask)
    row_gate.check(key, tag, res, bw["f32"], bw["f64"], ref.accum_skip(mask, state["seqs"]), report)
    return res


def _all_variants(key, ref, path):
    for prezeroed in (False, True):
        a = run_case(key, ref, path, rays=False, prezeroed=prezeroed)
        b = run_case(key, ref, path, rays=True, prezeroed=prezeroed)
        assert set(a) == set(b)


@pytest.mark.parametrize("path", PATHS, ids=PATH_IDS)
@pytest.mark.parametrize("name", list(SCENES))
def test_rows_of_every_scene_on_every_path(refs, name, path):
    ref = refs(name, lambda: Reference(*scene(*SCENES[name]), 3, BG3[2]))
    _all_variants(name, ref, path)


# (deg, M): every table that holds the degree's coefficients; the rest of a larger table receives exact zeros (the gate's column rule)
DEG_M = [(deg, M) for deg in range(4) for M in (1, 4, 9, 16, 25) if (deg + 1) ** 2 <= M]
PARAM_PATHS = [PATHS[0], PATHS[1]]                       # the bucketed replay and the re-tracing backward (option deterministic ends at M = 17)


@pytest.mark.parametrize("deg,M", DEG_M, ids=[f"deg{d}-M{m}" for d, m in DEG_M])
def test_rows_for_every_sh_degree_and_table(refs, deg, M):
    key = f"p570-deg{deg}-M{M}"
    ref = refs(key, lambda: Reference(*scene(*SCENES["p570"], M=M), deg, BG3[2]))
    if (deg + 1) ** 2 < M:
        assert not ref.backward(ref.f32_events)["f64"]["shs"][:, (deg + 1) ** 2:].any()
    for path in PARAM_PATHS:
        for rays in (False, True):
            run_case(key, ref, path, rays=rays)


@pytest.mark.parametrize("deg", [0, 3])
@pytest.mark.parametrize("bg", BG3[:2], ids=["bg000", "bg001"])      # ((0.3, 0.7, 0.2) is the background of every other case)
def test_rows_for_every_background(refs, bg, deg):
    key = f"p570-deg{deg}-bg{bg[2]:.0f}"
    ref = refs(key, lambda: Reference(*scene(*SCENES["p570"]), deg, bg))
    for path in PARAM_PATHS:
        run_case(key, ref, path, rays=True)


def test_rows_with_a_scale_modifier(refs):
    ref = refs("p570-mod1.3", lambda: Reference(*scene(*SCENES["p570"]), 3, BG3[2], mod=1.3))
    for path in PARAM_PATHS:
        for rays in (False, True):
            run_case("p570-mod1.3", ref, path, rays=rays)


def test_rows_of_s10k_on_the_default_path(refs):
    """10 000 Gaussians, 16 x 256 rays: the learnt tables, the 8-wave forward and rows that span buckets are live."""
    ref = refs("s10k", lambda: Reference(*row_gate.s10k_case(), 3, scenes.BG_DEFAULT))
    if ref.f32_events.mean() > MAX_MASKED:               # the float32 oracle's own event rays alone: the left half of the image
        ref = refs("s10k[:, :128]", lambda: Reference(*row_gate.s10k_case(128), 3, scenes.BG_DEFAULT))
    run_case("s10k", ref, PATHS[0], rays=False)
    run_case("s10k", ref, PATHS[0], rays=True)
