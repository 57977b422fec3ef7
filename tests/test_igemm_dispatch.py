"""dc_igemm's dispatcher, pinned without a GPU: which kernel (or which refusal) every problem of a deterministic sweep gets,
what the six probes answer for it, and the status / error text of dc_igemm on the refused ones.

dc_igemm_variant, the dc_igemm_*_ok / _parts probes and dc_igemm itself on a refused problem run on the host alone, so the sweep
needs no device; dc_igemm is never called on a problem the dry run accepts (that would launch).  tests/golden/igemm_dispatch.npz is
the recorded table (tools/capture_igemm_dispatch.py; tests/golden/README.md says at which commit) and the library under test must
reproduce it case for case and string for string.  The DCAMD_* switches are read once per process: the default environment is swept
in this process, each switch on a reduced grid in a child process (no GPU is opened: only ctypes and _lib.py are loaded there)."""
import ctypes
import hashlib
import importlib.util
import itertools
import os
import re
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "igemm_dispatch.npz")
FAKE = 1 << 20          # non-null, 16-byte aligned; never dereferenced on the host
F32, BF16, F16 = 0, 1, 2
NOT_CALLED = 1        # in place of a status where dc_igemm was not called (the dc_status codes are <= 0)
ENVS = [("default", None), ("DCAMD_NO_HALO", "1"), ("DCAMD_WS_PLAIN", "1"), ("DCAMD_NO_THIN", "1"), ("DCAMD_NO_MOSAIC", "1"),
        ("DCAMD_NO_PN", "1"), ("DCAMD_NO_XREG", "1"), ("DCAMD_NO_WS", "1"), ("DCAMD_PIPE_NO_WIDE", "1"), ("DCAMD_HALO_NO_STAG", "1"),
        ("DCAMD_PIPE_CHIP_TILES", "0")]
PROBES = ["dc_igemm_gn_fusable", "dc_igemm_side_ok", "dc_igemm_ln_ok", "dc_igemm_pn_ok", "dc_igemm_up4_ok"]     # bit i of `probes`
TAGS = ["invalid", "side-source-unsupported", "gn-not-fusable", "qstats-unsupported", "producer-groupnorm-unsupported",
        "up4-unsupported", "row-layernorm-unsupported"]
FAMILIES = [r"conv3_thin<\w+>", r"conv3_ws<\w+,gn>", r"conv3_ws<\w+>", r"conv3_halo<\w+,4w>", r"conv3_halo<\w+,8w>",
            r"conv3_halo<\w+,4w,pn>", r"conv3_halo<\w+,8w,pn>", r"conv3_up4<\w+,4w>", r"conv3_up4<\w+,8w>", r"conv3_up4<\w+,4w,pn>",
            r"igemm_pipe_up4<\w+,256x128,3st>", r"igemm_xreg<\w+,96xN>", r"igemm_pipe<\w+,128x128,2st>", r"igemm_pipe<\w+,256x128,3st>",
            r"igemm_wide8<\w+,256x256>", r"igemm<\w+,128x128>", r"igemm<\w+,128x32>"]


def _load_lib():
    """_lib.py alone (ctypes only), so that a child process pays for neither torch nor the package."""
    spec = importlib.util.spec_from_file_location("_dcamd_lib_only", os.path.join(ROOT, "diffusion-classifier_amd", "_lib.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# ---- the cases ------------------------------------------------------------------------------------------------------------------
def _base(dt, taps, stride, ups, H, W, C0, C1, Cout, tile_n, act, n_img):
    """A plain problem as the engine states it, or None where dc_igemm's own rules make the combination meaningless."""
    if taps == 1 and (stride != 1 or ups):
        return None
    if ups and (stride != 1 or H % 2 or W % 2):
        return None
    if act == 2 and (tile_n != 128 or Cout % 32):
        return None
    if (C0 % (32 if dt == F32 else 64)) or (C1 % (32 if dt == F32 else 64)):
        return None
    Ho, Wo = ((H - 1) // stride + 1, (W - 1) // stride + 1) if taps == 9 else (H, W)
    cout_out = Cout // 2 if act == 2 else Cout
    return dict(dtype=dt, taps=taps, stride=stride, upsample=ups, n_img=n_img, Hin=H, Win=W, Hout=Ho, Wout=Wo, src0=FAKE, C0=C0, ld0=C0,
                src1=FAKE if C1 else None, C1=C1, ld1=C1, W=FAKE, Cout=Cout, tile_n=tile_n, bias=FAKE, act=act, out=FAKE, out_dtype=dt,
                out_ld=cout_out, pn_groups=32, pn_eps=1e-5)


GEOM = [(9, 1, 0), (9, 2, 0), (9, 1, 1), (1, 1, 0)]
EXTENTS = [(e, e) for e in (2, 4, 8, 16, 32, 64, 128, 24)] + [(16, 32), (256, 1)]


def grid_cases(reduced=False):
    """The cross product of the plain problems (reduced: the smaller one swept under each environment switch)."""
    if reduced:
        axes = ((F32, BF16), GEOM, [(4, 4), (8, 8), (16, 16), (64, 64), (16, 32)], (64, 320), (0, 128), (16, 128, 1024), (128, 32), (0, 2), (1, 800))
    else:
        axes = ((F32, BF16, F16), GEOM, EXTENTS, (32, 64, 128, 320, 768), (0, 128), (3, 16, 128, 256, 320, 1024, 3072), (128, 32),
                (0, 1, 2, 3), (1, 16, 800))
    out = []
    for dt, (taps, stride, ups), (H, W), C0, C1, Cout, tile_n, act, n_img in itertools.product(*axes):
        c = _base(dt, taps, stride, ups, H, W, C0, C1, Cout, tile_n, act, n_img)
        if c is not None:
            out.append(c)
    return out


_PN = dict(pn_out=FAKE, pn_gamma=FAKE, pn_beta=FAKE, pn_cnt=FAKE, pn_ld=0, pn_silu=1)
_SIDE = dict(src2=FAKE, W2=FAKE, C2=128, ld2=128)
_GN = dict(gn_scale=FAKE, gn_shift=FAKE, gn_silu=1)


def _res(c, **kw):
    return dict(dict(residual=FAKE, res_dtype=c["dtype"], res_ld=c["out_ld"]), **kw)


def feature_cases():
    """Each opt-in feature on its own, and in the pairs the engine uses, on 3x3 and 1-tap bases."""
    out = []
    for dt, (H, W), C0, Cout, n_img in itertools.product((F32, BF16, F16), [(4, 4), (8, 8), (16, 16), (32, 32), (64, 64), (128, 128), (16, 32), (24, 24)],
                                                         (64, 128, 320), (16, 128, 320), (1, 16)):
        c = _base(dt, 9, 1, 0, H, W, C0, 0, Cout, 128, 0, n_img)
        c1 = _base(dt, 9, 1, 0, H, W, C0, 128, Cout, 128, 0, n_img)
        mods = [dict(qstats=FAKE), dict(_PN, qstats=FAKE), dict(_PN), dict(_PN, qstats=FAKE, out=None), dict(out=None),
                dict(_PN, qstats=FAKE, pn_groups=Cout // 24 or 1), dict(_PN, qstats=FAKE, pn_eps=0.0), dict(_PN, qstats=FAKE, pn_cnt=FAKE + 2),
                dict(_PN, qstats=FAKE, pn_ld=Cout + 4), dict(_PN, qstats=FAKE + 8), dict(_PN, qstats=FAKE, **_GN),
                dict(_SIDE), dict(_SIDE, **_GN), _res(c, **_SIDE), _res(c, **_SIDE, **_GN), dict(_SIDE, C2=24), dict(_SIDE, W2=None),
                dict(_SIDE, src2=FAKE + 4), dict(_SIDE, qstats=FAKE), dict(_GN), dict(_GN, qstats=FAKE), dict(gn_scale=FAKE), _res(c, **_GN),
                dict(out_dtype=F32), dict(out_dtype=F32, qstats=FAKE), _res(c), _res(c, res_dtype=F32 if dt != F32 else BF16),
                dict(out_ld=Cout + 4), _res(c, res_ld=Cout + 4), dict(bias=FAKE + 4), dict(out=FAKE + 4), dict(out=FAKE + 8, **_GN),
                dict(rowvec=FAKE, rowvec_ld=Cout), dict(rowvec=FAKE, rowvec_ld=Cout + 2), dict(gate=FAKE, gate_ld=Cout),
                dict(ln_eps=1e-5), dict(up4=1)]
        out += [dict(c, **m) for m in mods]
        out += [dict(c1, **m) for m in (dict(_GN), dict(qstats=FAKE), dict(_PN, qstats=FAKE), dict(_SIDE), dict(_GN, qstats=FAKE))]
        # the upsample conv: Hin / Win are the upsampled extents
        u = _base(dt, 9, 1, 1, 2 * H, 2 * W, C0, 0, Cout, 128, 0, n_img)
        out += [dict(u, **m) for m in (dict(up4=1), dict(up4=1, qstats=FAKE), dict(_PN, up4=1, qstats=FAKE), dict(_PN, up4=1), dict(_PN, up4=1, qstats=FAKE, out=None),
                                       dict(up4=1, out_dtype=F32), dict(up4=1, out_ld=Cout + 4), _res(u, up4=1), dict(up4=1, tile_n=32), dict(qstats=FAKE),
                                       dict(_PN, qstats=FAKE), dict(_GN), dict(_SIDE), dict(up4=1, src1=FAKE, C1=128, ld1=128))]
    for dt, (H, W), C0, Cout, n_img, act in itertools.product((F32, BF16, F16), [(16, 16), (256, 1)], (128, 256, 768), (256, 1024, 3072), (1, 16, 800), (0, 2, 3)):
        g = _base(dt, 1, 1, 0, H, W, C0, 0, Cout, 128, act, n_img)
        mods = [dict(ln_eps=1e-5), dict(ln_eps=1e-5, out_dtype=F32), dict(ln_eps=1e-5, out_ld=g["out_ld"] + 4), dict(ln_eps=1e-5, src1=FAKE, C1=128, ld1=128),
                dict(out_dtype=F32), _res(g), _res(g, res_dtype=F32 if dt != F32 else BF16), dict(out_ld=g["out_ld"] + 4), dict(bias=FAKE + 4),
                dict(gate=FAKE, gate_ld=g["out_ld"]), dict(rowvec=FAKE, rowvec_ld=g["out_ld"]), dict(qstats=FAKE), dict(_GN), dict(_SIDE), dict(up4=1),
                dict(_PN, qstats=FAKE), dict(ld0=C0 + 8), dict(ld0=C0 + 4), dict(ld0=C0 - 64)]
        out += [dict(g, **m) for m in mods]
    # what the DC_REQUIRE block refuses
    b = _base(BF16, 9, 1, 0, 16, 16, 64, 0, 128, 128, 0, 1)
    out += [dict(b, **m) for m in (dict(dtype=7), dict(taps=4), dict(stride=3), dict(tile_n=64), dict(src0=None), dict(W=None), dict(C0=32), dict(C0=0),
                                   dict(C1=64), dict(n_img=0), dict(Hout=15), dict(act=4), dict(act=2, Cout=48), dict(src0=FAKE + 8), dict(ld0=68), dict(out_ld=64),
                                   _res(b, res_ld=64), dict(rowvec=FAKE, rowvec_ld=64), dict(gate=FAKE, gate_ld=64), dict(n_img=1 << 24, Hin=128, Win=128, Hout=128, Wout=128),
                                   dict(taps=1, stride=2), dict(upsample=1, Hin=15, Win=15, Hout=15, Wout=15))]
    return out


def all_cases(reduced=False):
    return grid_cases(reduced) + feature_cases()


def cases_digest(cases):
    """The fixture names the generator it was captured with: a change of the cases must come with a new capture."""
    h = hashlib.sha256()
    for c in cases:
        h.update(repr(sorted(c.items())).encode())
    return h.hexdigest()


# ---- the sweep ------------------------------------------------------------------------------------------------------------------
def sweep(cases):
    """Per case: the variant string, the five yes / no probes as bits, the quad-statistics part count and, for a refusal, dc_igemm's
    status (else NOT_CALLED) and error text (else "")."""
    L = _load_lib()
    lib = L.lib()
    probes = [getattr(lib, n) for n in PROBES]
    n = len(cases)
    variant, err = [None] * n, [""] * n
    bits, parts, rc = np.zeros(n, np.uint8), np.zeros(n, np.int32), np.full(n, NOT_CALLED, np.int16)
    for i, c in enumerate(cases):
        p = L.IgemmParams(**{k: v for k, v in c.items() if v is not None})
        v = lib.dc_igemm_variant(p).decode()
        variant[i] = v
        b = 0
        for j, fn in enumerate(probes):
            r = fn(p)
            assert r in (0, 1), (PROBES[j], r)
            b |= r << j
        bits[i] = b
        parts[i] = lib.dc_igemm_qstats_parts(p)
        if v in TAGS:        # refused: dc_igemm stops before any launch
            rc[i] = lib.dc_igemm(p, None)
            err[i] = lib.dc_last_error().decode()
            assert rc[i] < 0, c
    return dict(variant=variant, probes=bits, parts=parts, rc=rc, err=err)


def sweep_env(name, value, reduced):
    """The sweep in a child process with one switch set (the library reads them once per process)."""
    import tempfile
    env = {k: v for k, v in os.environ.items() if not k.startswith("DCAMD_") or k == "DCAMD_LIB"}
    if value is not None:
        env[name] = value
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "sweep.npz")
        subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "reduced" if reduced else "full", path], check=True, env=env, timeout=600)
        with np.load(path) as z:
            return dict(variant=z["variant"].tolist(), probes=z["probes"], parts=z["parts"], rc=z["rc"], err=z["err"].tolist())


def capture():
    """Every environment's table: {env name: sweep result}; 'default' on the full cases, the switches on the reduced ones."""
    assert not [k for k in os.environ if k.startswith("DCAMD_") and k != "DCAMD_LIB"], "capture / compare in a clean environment"
    return {name: (sweep(all_cases()) if value is None else sweep_env(name, value, True)) for name, value in ENVS}


def encode(tables):
    """Distinct strings once, integer codes per case."""
    strings = sorted({s for t in tables.values() for s in t["variant"] + t["err"]})
    code = {s: i for i, s in enumerate(strings)}
    out = {"strings": np.array(strings), "digest_full": np.array(cases_digest(all_cases())), "digest_reduced": np.array(cases_digest(all_cases(True)))}
    for name, t in tables.items():
        out[name + "/variant"] = np.array([code[s] for s in t["variant"]], np.uint16)
        out[name + "/err"] = np.array([code[s] for s in t["err"]], np.uint16)
        out[name + "/probes"] = t["probes"].astype(np.uint8)
        out[name + "/parts"] = t["parts"].astype(np.uint16)
        assert (t["parts"] >= 0).all() and (t["parts"] < 65536).all()
        out[name + "/rc"] = t["rc"].astype(np.int16)
    return out


def load_fixture():
    with np.load(FIXTURE) as z:
        strings = z["strings"].tolist()
        tables = {}
        for name, _ in ENVS:
            tables[name] = dict(variant=[strings[i] for i in z[name + "/variant"]], err=[strings[i] for i in z[name + "/err"]],
                                probes=z[name + "/probes"], parts=z[name + "/parts"].astype(np.int32), rc=z[name + "/rc"])
        return tables, str(z["digest_full"]), str(z["digest_reduced"])


# ---- the tests ------------------------------------------------------------------------------------------------------------------
def test_fixture_covers_every_route_refusal_and_probe_answer():
    tables, dfull, dred = load_fixture()
    assert dfull == cases_digest(all_cases()) and dred == cases_digest(all_cases(True)), "the case generator changed: capture again"
    assert len(tables["default"]["variant"]) == len(all_cases()) > 150000
    seen = {v for t in tables.values() for v in t["variant"]}
    for fam in FAMILIES:
        assert any(re.fullmatch(fam, v) for v in seen), fam
    for tag in TAGS:
        assert tag in seen, tag
    assert all(any(re.fullmatch(fam, v) for fam in FAMILIES) or v in TAGS for v in seen), seen       # and nothing this file does not know
    d = tables["default"]
    for j, name in enumerate(PROBES):
        ans = (d["probes"] >> j) & 1
        assert ans.min() == 0 and ans.max() == 1, name
    assert len(set(d["parts"].tolist())) >= 4, set(d["parts"].tolist())       # 0 and at least three part counts
    refused = np.array([v in TAGS for v in d["variant"]])
    assert ((d["rc"] != NOT_CALLED) == refused).all() and all(bool(e) == r for e, r in zip(d["err"], refused))
    # every switch changes something on its grid, or its child sweep pins nothing
    red = tables["DCAMD_NO_HALO"]
    assert len(red["variant"]) == len(all_cases(True))


def _compare(name, got, want, cases):
    bad = [i for i in range(len(cases)) if (got["variant"][i], got["err"][i], int(got["probes"][i]), int(got["parts"][i]), int(got["rc"][i])) !=
           (want["variant"][i], want["err"][i], int(want["probes"][i]), int(want["parts"][i]), int(want["rc"][i]))]
    msg = "\n".join(f"{cases[i]}\n  got  {got['variant'][i]!r} probes={int(got['probes'][i]):05b} parts={int(got['parts'][i])} rc={int(got['rc'][i])} {got['err'][i]!r}"
                    f"\n  want {want['variant'][i]!r} probes={int(want['probes'][i]):05b} parts={int(want['parts'][i])} rc={int(want['rc'][i])} {want['err'][i]!r}" for i in bad[:10])
    assert not bad, f"{name}: {len(bad)} of {len(cases)} cases differ from the recorded dispatch\n{msg}"


def test_default_environment_matches_recorded_dispatch():
    tables, _, _ = load_fixture()
    cases = all_cases()
    got = sweep_env("default", None, False) if [k for k in os.environ if k.startswith("DCAMD_") and k != "DCAMD_LIB"] else sweep(cases)
    _compare("default", got, tables["default"], cases)


def test_each_switch_matches_recorded_dispatch():
    tables, _, _ = load_fixture()
    cases = all_cases(True)
    for name, value in ENVS[1:]:
        _compare(name, sweep_env(name, value, True), tables[name], cases)
        assert any(a != b for a, b in zip(tables[name]["variant"], _reduced_default(tables))) or \
            (tables[name]["probes"] != _reduced_default_probes(tables)).any(), f"{name} changes nothing on the reduced grid"


def test_instance_agrees_with_variant_on_every_halo_conv(monkeypatch):
    """dc_igemm_instance against dc_igemm_variant over the whole sweep, default environment: a conv3_halo<...> / conv3_up4<...> problem runs
    conv3_halo_kernel in the variant's dtype and wave count, with 4 taps exactly for the four-phase form and pn exactly where the variant
    says so, and a producer-side-GroupNorm launch is one of the four instances that exist for it."""
    monkeypatch.delenv("DCAMD_HALO_NO_STAG", raising=False)
    L = _load_lib()
    lib = L.lib()
    n, pn_seen = 0, set()
    for c in all_cases():
        p = L.IgemmParams(**{k: v for k, v in c.items() if v is not None})
        v = re.fullmatch(r"conv3_(halo|up4)<(\w+),([48])w(,pn)?>", lib.dc_igemm_variant(p).decode())
        if not v:
            continue
        inst = lib.dc_igemm_instance(p, None).decode()
        k = re.fullmatch(r"conv3_halo_kernel<(\w+),(\d+),(\d+),(\d+)(,stag)?(,pn)?>", inst)
        assert k, (c, v[0], inst)
        up4 = v[1] == "up4"
        key = (int(k[2]), int(k[3]), int(k[4]), bool(k[5]), bool(k[6]))
        assert k[1] == v[2] and key[0] == int(v[3]) and key[1] == (4 if up4 else 9) and key[4] == bool(v[4]) and up4 == bool(c.get("up4")), (c, v[0], inst)
        if key[4]:
            want = ((4, 4, 1, False, True) if up4 else (4, 9, 1, False, True)) if key[0] == 4 else \
                {(8, 8): (8, 9, 0, True, True), (4, 4): (8, 9, 2, True, True)}.get((c["Hin"], c["Win"]))
            assert key == want, (c, v[0], inst)
            pn_seen.add(key)
        n += 1
    assert n > 10000 and len(pn_seen) == 4, (n, pn_seen)


def _reduced_index():
    """Positions of the reduced cases inside the full list (the reduced grid is a subset of the full one; the feature cases are shared)."""
    pos = {repr(sorted(c.items())): i for i, c in enumerate(all_cases())}
    return [pos[repr(sorted(c.items()))] for c in all_cases(True)]


def _reduced_default(tables):
    return [tables["default"]["variant"][i] for i in _reduced_index()]


def _reduced_default_probes(tables):
    return tables["default"]["probes"][_reduced_index()]


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--child":
        t = sweep(all_cases(sys.argv[2] == "reduced"))
        np.savez(sys.argv[3], variant=np.array(t["variant"]), err=np.array(t["err"]), probes=t["probes"], parts=t["parts"], rc=t["rc"])
