"""GPU: every GroupNorm / LayerNorm kernel and launch sequence of csrc/norms.hip against an fp64 reference over EVERY output element with
a derived per-element bound (tests/norm_cases.py: the cases, the operands, the reference, the bound and the checker;
tests/test_norm_cases.py pins their routing and holds the checker against planted faults on the host).

Every case: the operands are rounded to the compute type first and the reference is formed from exactly those; the variant string is
asserted on the real pointers before the launch; outputs (y, or out_scale / out_shift) are pre-filled with a sentinel and a guard region
behind them — and behind dc_groupnorm_ws_floats of the workspace — must still hold it bit for bit; sources read through a map have a sample
no map names; the pad columns of a modulation table hold NaN.  The tolerances of test_gpu_ops.py's norm tests stay as a second, outer
assertion.  DCAMD_GN_SPAN / DCAMD_GN_NO_WAVE are read once per process: this module runs the cases whose `env` is the process's own, and
one child interpreter per switch (a fresh pytest process, never an exec) runs the others."""
import os
import re
import subprocess
import sys
import tempfile
import time

import pytest
import torch

import norm_cases as N
from diffusion_classifier_amd import _lib as L

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
T0 = time.time()
ACTIVE = {k: os.environ[k] for k in N.SWITCHES if k in os.environ}            # the switches this process runs under
MINE = [c for c in N.CASES if c["env"] == ACTIVE]
PEER_DIR = os.environ.get("NORM_CASES_PEER_DIR")                               # set by the parent of a switch's child: what the other route gave
# test_gpu_ops.py: test_groupnorm (f16 by the same rule: 8 x 2^-11 x 2), test_layernorm_plain_and_adaln (x 3 with modulation)
OUTER_GN = {N.F32: 2e-4, N.BF16: 6e-2, N.F16: 8e-3}
OUTER_LN = {N.F32: 2e-5, N.BF16: 5e-2, N.F16: 8e-3}


@pytest.fixture(scope="module", autouse=True)
def _wall_time():
    yield
    print(f"\ntest_gpu_norms.py [{ACTIVE or 'default'}]: {len(MINE)} cases, wall time {time.time() - T0:.1f} s")


def _es(c):
    return 4 if c["dtype"] == N.F32 else 2


def device_operands(c, o):
    """{name: device tensor} (the tensors must outlive the launch)."""
    td = N.TD[c["dtype"]]
    if c["kind"] == "gn":
        d = {"x": o["x0"].to(td).to(DEV), "gamma": o["gamma"].to(DEV), "beta": o["beta"].to(DEV)}
        if "x1" in o:
            d["x1"] = o["x1"].to(td).to(DEV)
        for f in ("map0", "map1", "qstats"):
            if f in o:
                d[f] = o[f].contiguous().to(DEV)
        return d
    d = {"x": o["x"].to(td).to(DEV)}
    if "gamma" in o:       # gamma_off floats into its allocation: the 4-byte misalignment that forces ln_kernel
        g = torch.zeros(c["C"] + 4)
        g[c["gamma_off"]: c["gamma_off"] + c["C"]] = o["gamma"]
        d["gamma"], d["beta"] = g.to(DEV), o["beta"].to(DEV)
    if "scale" in o:
        if c["table6"]:
            d["table"] = o["table"].contiguous().to(DEV)
        else:
            for f in ("scale", "shift"):
                t = torch.full((o[f].shape[0] * c["mod_ld"] + 4,), float("nan"))
                t[c["mod_off"]: c["mod_off"] + o[f].shape[0] * c["mod_ld"]].view(-1, c["mod_ld"])[:, : c["C"]] = o[f]
                d[f] = t.to(DEV)
        if "mod_map" in o:
            d["mod_map"] = o["mod_map"].to(DEV)
    return d


def pointers(c, d, first=0):
    """{pointer field: address} of the launch that starts at sample `first`: through the map where there is one, else by offset."""
    es = _es(c)
    if c["kind"] == "gn":
        HW, C0, C1, u = c["HW"], c["C"], c["C1"], c["use"]
        p = {"gamma": d["gamma"].data_ptr(), "beta": d["beta"].data_ptr()}
        src0 = 0 if "map0" in u else first
        p["x"] = d["x"].data_ptr() + src0 * HW * C0 * es
        if "map0" in u:
            p["map0"] = d["map0"].data_ptr() + 4 * first
        if "qstats" in u:
            p["qstats"] = d["qstats"].data_ptr() + src0 * c["qparts"] * (C0 // 4) * 8
        if "x1" in u:
            p["x1"] = d["x1"].data_ptr() + (0 if "map1" in u else first) * HW * C1 * es
        if "map1" in u:
            p["map1"] = d["map1"].data_ptr() + 4 * first
        return p
    C, rps, u = c["C"], c["rows_per_sample"], c["use"]
    p = {"x": d["x"].data_ptr() + first * rps * C * es}
    if "affine" in u:
        p["gamma"], p["beta"] = d["gamma"].data_ptr() + 4 * c["gamma_off"], d["beta"].data_ptr()
    if "mod" in u:
        off = 0 if "mod_map" in u else first * c["mod_ld"] * 4
        if c["table6"]:
            p["shift"], p["scale"] = d["table"].data_ptr() + off, d["table"].data_ptr() + 4 * C + off
        else:
            p["scale"], p["shift"] = d["scale"].data_ptr() + 4 * c["mod_off"] + off, d["shift"].data_ptr() + 4 * c["mod_off"] + off
        if "mod_map" in u:
            p["mod_map"] = d["mod_map"].data_ptr() + 4 * first
    return p


def launch(c, d, first=0, count=None):
    """Launch samples [first, first + count) of the case into fresh sentinel-filled buffers; returns them on the CPU (guards checked)."""
    lib = L.lib()
    if c["kind"] == "gn":
        sub = dict(c, n=c["n"] - first if count is None else count)
    else:
        rps = c["rows_per_sample"]
        sub = dict(c, rows=c["rows"] - first * rps if count is None else min(count * rps, c["rows"] - first * rps))
    outs = N.new_outputs(sub, DEV)
    p = pointers(c, d, first)
    for (label, _, _), buf in zip(N.out_shapes(sub), outs):
        p[label] = buf.data_ptr()
    if c["kind"] == "gn":
        nws = lib.dc_groupnorm_ws_floats(sub["n"], c["groups"], c["splits"])
        assert nws == N.ws_floats(sub)
        ws = torch.full((nws + N.GUARD,), N.SENTINEL, device=DEV)
        p["ws"] = ws.data_ptr()
        params = L.GroupnormParams(**N.gn_fields(sub, p))
        variant = lib.dc_groupnorm_variant(params).decode()
        assert variant == c["expect"], (c["name"], variant)
        L.check(lib.dc_groupnorm(params, L.stream_ptr()), "dc_groupnorm")
        torch.cuda.synchronize()
        assert N.guard_intact(ws.cpu(), nws) == 0, f"{c['name']}: the workspace was written behind dc_groupnorm_ws_floats"
    else:
        params = L.LayernormParams(**N.ln_fields(sub, p))
        variant = lib.dc_layernorm_variant(params).decode()
        assert variant == c["expect"], (c["name"], variant)
        L.check(lib.dc_layernorm(params, L.stream_ptr()), "dc_layernorm")
        torch.cuda.synchronize()
    return sub, [b.cpu() for b in outs]


def _body(sub, bufs):
    return [b[: b.numel() - N.GUARD].view(shape) for b, (_, shape, _) in zip(bufs, N.out_shapes(sub))]


def _differ(a, b):
    return int((N._bits(a.contiguous()) != N._bits(b.contiguous())).sum())


@pytest.mark.parametrize("c", MINE, ids=lambda c: c["name"])
def test_norm_kernel_against_fp64_reference(c):
    t0 = time.time()
    o = N.make_operands(c)
    refs = N.reference(c, o)
    d = device_operands(c, o)
    _, bufs = launch(c, d)
    problems, worst = N.check_outputs(c, bufs, refs)
    outer_tol = (OUTER_GN if c["kind"] == "gn" else OUTER_LN)[c["dtype"]] * (3 if "mod" in c["use"] else 1)
    if "stats_only" in c["use"]:
        outer_tol = OUTER_GN[N.F32]       # out_scale / out_shift are fp32 whatever the tensor's type
    outer = err_torch = 0.0
    for got, (_, ref, _, _), t32 in zip(_body(c, bufs), refs, N.torch_fp32(c, o)):
        outer = max(outer, float((got.double() - ref).abs().max()))
        err_torch = max(err_torch, float((t32.double() - ref).abs().max()))
    print(f"{c['name']} [{N.family(c)} {N.DTN[c['dtype']]}] {c['tag']}: worst err / bound {worst:.4f}, max err {outer:.2e} (torch fp32 {err_torch:.2e}); {time.time() - t0:.2f} s")
    assert not problems, (c["name"], problems)
    assert outer < max(4 * err_torch, outer_tol), (c["name"], outer, err_torch)      # test_groupnorm_with_large_offsets_f32's rule
    if PEER_DIR and os.path.exists(os.path.join(PEER_DIR, c["name"] + ".pt")):
        # the same problem on the route the parent process took (no switch set): gn_span_kernel folds the records in gn_image_kernel's
        # order and must agree bit for bit; elsewhere both lie inside the bound (the parent checked its own)
        peer = torch.load(os.path.join(PEER_DIR, c["name"] + ".pt"))
        differ = sum(_differ(a, b) for a, b in zip(bufs, peer))
        print(f"{c['name']}: {differ} elements differ from the other route's")
        if c["expect"] == "span":
            assert differ == 0, f"{c['name']}: span and image differ in {differ} elements"


@pytest.mark.parametrize("name", [n for n in N.INDEPENDENT if N.by_name(n)["env"] == ACTIVE])
def test_a_sample_does_not_depend_on_how_many_share_the_launch(name):
    """All samples / rows in one launch, then one sample alone and all but the first (through the map, or by pointer offset): y and
    out_scale / out_shift bit identical — what gn_route's and ln_route's comments promise and dc_groupnorm_splits exists for."""
    c = N.by_name(name)
    d = device_operands(c, N.make_operands(c))
    _, full = launch(c, d)
    full = _body(c, full)
    per = 1 if c["kind"] == "gn" else c["rows_per_sample"]
    total = c["n"] if c["kind"] == "gn" else c["n_samples"]
    assert total >= 3
    for first, count in ((total - 2, 1), (1, None)):
        sub, part = launch(c, d, first, count)
        for a, b in zip(_body(sub, part), full):
            want = b[first * per: first * per + a.shape[0]]
            assert a.shape == want.shape and a.shape[0] > 0
            differ = _differ(a, want)
            assert differ == 0, f"{name}: samples from {first} on, launched {'alone' if count else 'without the first'}: {differ} elements differ"


@pytest.mark.parametrize("name", [c["name"] for c in MINE if c["tag"] == "probe"])
def test_the_applied_affine_is_the_emitted_one_bit_for_bit(name):
    """gn_image_kernel / gn_span_kernel from records against gn_qaffine_kernel's out_scale / out_shift from the same records
    (gn_fold_rec: "must agree bit for bit"): where x is 0 the output is the shift, where x is 1 it is fl(scale + shift), whether or not
    the compiler contracts x * scale + shift."""
    c = N.by_name(name)
    assert c["dtype"] == N.F32 and not c["silu"]
    o = N.make_operands(c)
    assert bool((o["x0"][:, 0] == 0).all()) and bool((o["x0"][:, 1] == 1).all())
    d = device_operands(c, o)
    _, bufs = launch(c, d)
    y = _body(c, bufs)[0]
    q = dict(c, use=c["use"] | {"stats_only"}, expect="qaffine")
    _, aff = launch(q, d)
    scale, shift = _body(q, aff)
    assert _differ(y[:, 0], shift) == 0
    assert _differ(y[:, 1], scale + shift) == 0


@pytest.mark.parametrize("name", [n for n in N.REPEAT_CASES if N.by_name(n)["env"] == ACTIVE])
def test_norm_kernels_are_deterministic_at_size(name):
    c = N.by_name(name)
    d = device_operands(c, N.make_operands(c))
    outs = []
    for _ in range(3):
        torch.randn(1 << 22, device=DEV).sum()
        outs.append(launch(c, d)[1])
    for o2 in outs[1:]:
        differ = sum(_differ(a, b) for a, b in zip(o2, outs[0]))
        assert differ == 0, f"{name}: a repeated launch differs in {differ} elements"


@pytest.mark.parametrize("switch", N.SWITCHES)
def test_switch_cases_in_a_child_interpreter_and_both_routes_agree(switch):
    """The cases of one switch: first the same problems here, on the route they take with no switch set (gn_image_kernel for the span
    cases, gn_wave_kernel for the DCAMD_GN_NO_WAVE ones), checked against the same bound and kept; then ONE fresh pytest process with the
    switch set runs this module's case, independence and probe tests and compares with what was kept."""
    if ACTIVE:       # this process is such a child (or was started with a switch set): its own cases are the parametrised tests above
        return
    env = {switch: "1"}
    cases = [c for c in N.CASES if c["env"] == env]
    other = {"DCAMD_GN_SPAN": {"image"}, "DCAMD_GN_NO_WAVE": {"wave"}}[switch]
    with tempfile.TemporaryDirectory() as peer_dir:
        kept = 0
        for c in cases:
            p = dict(c, env={})
            o = N.make_operands(p)
            d = device_operands(p, o)
            p["expect"] = L.lib().dc_groupnorm_variant(L.GroupnormParams(**N.gn_fields(p, N.fake_ptrs(p)))).decode()
            assert p["expect"] in other, (c["name"], p["expect"])
            _, bufs = launch(p, d)
            problems, worst = N.check_outputs(p, bufs, N.reference(p, o))
            assert not problems, (c["name"], p["expect"], problems)
            torch.save(bufs, os.path.join(peer_dir, c["name"] + ".pt"))
            kept += 1
        assert kept == len(cases)
        child_env = dict({k: v for k, v in os.environ.items() if k not in N.SWITCHES}, NORM_CASES_PEER_DIR=peer_dir, **env)
        n_indep, n_probe = sum(N.by_name(n)["env"] == env for n in N.INDEPENDENT), sum(c["tag"] == "probe" for c in cases)
        select = " or ".join(["against_fp64_reference"] + ["share_the_launch"] * bool(n_indep) + ["bit_for_bit"] * bool(n_probe))      # (no empty parameter sets)
        r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-s", "-m", "gpu", "-p", "no:cacheprovider", "-k", select],
                           env=child_env, capture_output=True, text=True, timeout=900)
    print("\n".join(line for line in r.stdout.splitlines() if "err / bound" in line or "differ" in line or "wall time" in line))
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    m = re.search(r"(\d+) passed", r.stdout)
    want = len(cases) + n_indep + n_probe
    assert m and int(m.group(1)) == want and "failed" not in r.stdout and "skipped" not in r.stdout, (want, r.stdout[-500:])
    assert len(re.findall(r"elements differ from the other route's", r.stdout)) == len(cases)
