"""dc_groupnorm's and dc_layernorm's dispatchers, pinned without a GPU: which launch sequence every problem of a deterministic sweep
gets, that the answer never depends on the number of samples / rows in the launch, and the status / error text of the refused ones.

dc_groupnorm_variant / dc_layernorm_variant and dc_groupnorm / dc_layernorm themselves on a refused problem run on the host alone;
neither entry point is ever called on a problem the variant accepts (that would launch).  The expectation is NOT recorded from the
library: `gn_ladder` and `ln_ladder` below restate, in Python, the fall-through ladders dc_groupnorm and dc_layernorm had before
gn_choose / ln_route replaced them (thresholds as literals, conditions in the ladder's order, n where the ladder had n), so a moved
threshold or a reordered condition in csrc/norms.hip shows here as a changed route.  DCAMD_GN_NO_WAVE / DCAMD_GN_SPAN are read once
per process: the default environment is swept in this process, each switch in a child process (only ctypes and _lib.py load there)."""
import collections
import importlib.util
import itertools
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 1 << 20          # non-null, 16-byte aligned; never dereferenced on the host
F32, BF16, F16 = 0, 1, 2
OK, ERR_ARG, ERR_SHAPE, ERR_DTYPE = 0, -1, -2, -3
GN_ROUTES = ["qaffine", "stats", "wave", "span", "qfold+span", "image", "stats+apply", "qfold+apply"]
ENVS = [("default", None), ("DCAMD_GN_NO_WAVE", "1"), ("DCAMD_GN_SPAN", "1")]


def _load_lib():
    """_lib.py alone (ctypes only), so that a child process pays for neither torch nor the package."""
    spec = importlib.util.spec_from_file_location("_dcamd_lib_only", os.path.join(ROOT, "diffusion-classifier_amd", "_lib.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# ---- GroupNorm: the ladder restated ------------------------------------------------------------------------------------------------
def gn_ladder(c, no_wave=False, span_all=False):
    """(route, status, piece of the error text) for a case dict: the DC_REQUIREs in their order, then the fall-through ladder with its
    LDS arithmetic and its grid-size terms in n."""
    dt, n, HW, C0, C1, groups, splits, qparts = c["dtype"], c["n"], c["HW"], c["C"], c["C1"], c["groups"], c["splits"], c["qparts"]
    qstats, stats_only = c["qstats"] is not None, c["y"] is None
    es = 4 if dt == F32 else 2
    epc = 16 // es
    C = C0 + C1
    if None in (c["x"], c["gamma"], c["beta"], c["ws"]):
        return "invalid", ERR_ARG, "null pointer"
    if stats_only and not (c["out_scale"] and c["out_shift"] and (groups <= 64 or qstats)):
        return "invalid", ERR_ARG, "statistics-only mode needs"
    if groups <= 0 or C % groups:
        return "invalid", ERR_SHAPE, f"C={C} groups={groups}"
    if C0 <= 0 or C0 % epc or C1 < 0 or C1 % epc:
        return "invalid", ERR_SHAPE, f"C0={C0} C1={C1}"
    if n <= 0 or HW <= 0 or splits <= 0 or splits > HW:
        return "invalid", ERR_SHAPE, "n/HW/splits"
    if (C1 > 0) != (c["x1"] is not None):
        return "invalid", ERR_ARG, "x1/C1 mismatch"
    if dt != c["out_dtype"]:
        return "invalid", ERR_DTYPE, "in/out dtype must match"
    if qstats and not (C1 == 0 and qparts > 0 and HW % qparts == 0 and (C // groups) % 4 == 0 and c["qstats"] % 8 == 0):
        return "invalid", ERR_ARG, "qstats needs"
    CP = C // epc
    TPR = 1
    while TPR < CP and TPR < 256:
        TPR <<= 1
    if 2 * (256 // TPR) * C * 4 > 64 * 1024:
        return "invalid", ERR_SHAPE, f"C={C} too large"
    if splits * n >= 1 << 31:
        return "invalid", ERR_SHAPE, "grid too large"
    if stats_only and qstats:
        return ("qaffine", OK, "") if groups <= 4096 else ("invalid", ERR_SHAPE, f"groups={groups}")
    if dt not in (F32, BF16, F16):       # every launch sequence but qaffine ends in a dtype ladder with this refusal
        return "invalid", ERR_DTYPE, f"dtype {dt}"
    if stats_only:
        return "stats", OK, ""
    img_bytes = HW * C * es
    if not no_wave and not qstats and CP <= 64 and n < 1 << 30:
        tpr = 1
        while tpr < CP:
            tpr <<= 1
        plw = 64 // tpr
        nch = (HW + plw - 1) // plw
        if nch <= 32 and 4 * (2 * C + 2 * groups) * 4 <= 64 * 1024:
            return "wave", OK, ""
    qsplit = qstats and img_bytes >= 1 << 20
    chunks = HW * CP
    if (span_all or qsplit) and qstats and C1 == 0 and CP <= 256 and CP & (CP - 1) == 0 and chunks % 1024 == 0 and groups <= 2048 and \
            n * (chunks // 1024) < 1 << 31:
        return ("qfold+span" if qsplit or qparts * (C >> 2) > 8 * 256 else "span"), OK, ""
    if not qsplit and img_bytes <= 4 << 20 and CP <= 512 and groups <= 512 and n < 1 << 30:
        return "image", OK, ""
    return ("qfold+apply" if qstats else "stats+apply"), OK, ""


def gn_case(lib, dt, n, HW, C0, C1, groups, quad, stats_only):
    """A problem as the engine states it: splits from dc_groupnorm_splits, one quad-record part per 128 pixels."""
    c = dict(x=FAKE, x1=FAKE if C1 else None, y=None if stats_only else FAKE, dtype=dt, out_dtype=dt, n=n, HW=HW, C=C0, C1=C1, groups=groups,
             silu=1, splits=lib.dc_groupnorm_splits(n, HW, C0 + C1), eps=1e-5, gamma=FAKE, beta=FAKE, ws=FAKE,
             out_scale=FAKE if stats_only else None, out_shift=FAKE if stats_only else None,
             qstats=FAKE if quad else None, qparts=max(1, HW // 128) if quad else 0)
    return c


def gn_grid(lib):
    """Pairs of cases that differ in n alone."""
    axes = ((F32, BF16, F16), (10, 16, 64, 256, 1024, 4096, 16384, 65536), (32, 64, 128, 256, 320, 384, 768, 1024, 2048), (0, 128), (32, 8, 96),
            (False, True), (False, True))
    return [tuple(gn_case(lib, dt, n, HW, C0, C1, groups, quad, so) for n in (1, 700)) for dt, HW, C0, C1, groups, quad, so in itertools.product(*axes)]


def gn_extra(lib):
    """What the grid does not reach: the remaining DC_REQUIREs, an unknown dtype, and the grid-size guards (which move a problem to the next
    route of the ladder from 2^30 samples / 2^31 workgroups on, and only there)."""
    def b(**over):
        return dict(gn_case(lib, BF16, 4, 256, 64, 0, 32, False, False), **over)

    def q(**over):
        return dict(gn_case(lib, BF16, 4, 16384, 256, 0, 32, True, False), **over)

    return [b(x=None), b(ws=None), b(n=0), b(HW=0), b(splits=0), b(splits=257), b(x1=FAKE), b(C1=128), b(out_dtype=F16), b(dtype=7, out_dtype=7),
            b(C1=-8), b(C=0), b(C=60), b(groups=0), b(groups=24), q(qstats=FAKE + 4), q(qparts=0), q(qparts=100), q(groups=128), q(C1=128, x1=FAKE),
            b(y=None, out_scale=FAKE), b(y=None, out_scale=FAKE, out_shift=FAKE, groups=8), b(y=None, out_scale=FAKE, out_shift=FAKE, C=1024, groups=128),
            b(n=1 << 26, HW=16384, splits=64), b(C=8192), b(C=16384), b(dtype=F32, out_dtype=F32, C=16384),
            b(n=(1 << 30) - 1, HW=16), b(n=1 << 30, HW=16), b(n=1 << 30, HW=4096, splits=1), b(n=(1 << 30) - 1, HW=4096, splits=1),
            q(n=1 << 22), q(n=(1 << 22) - 1), q(n=1 << 30, HW=1024, splits=1, qparts=8), q(n=1 << 24, HW=1024, C=512, qparts=8)]


def gn_sweep(lib_mod, cases):
    lib = lib_mod.lib()
    out = []
    for c in cases:
        p = lib_mod.GroupnormParams(**{k: v for k, v in c.items() if v is not None})
        out.append(lib.dc_groupnorm_variant(p).decode())
    return out


def _flat(pairs):
    return [c for pair in pairs for c in pair]


def _child_sweep(name, value):
    env = {k: v for k, v in os.environ.items() if not k.startswith("DCAMD_") or k == "DCAMD_LIB"}
    if value is not None:
        env[name] = value
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "sweep.json")
        subprocess.run([sys.executable, os.path.abspath(__file__), "--child", path], check=True, env=env, timeout=600)
        with open(path) as f:
            return json.load(f)


def _gn_tables():
    """{env name: (cases, names the library gives, names the ladder gives)} on the grid followed by the extra cases."""
    L = _load_lib()
    cases = _flat(gn_grid(L.lib())) + gn_extra(L.lib())
    clean = not [k for k in os.environ if k.startswith("DCAMD_") and k != "DCAMD_LIB"]
    out = {}
    for name, value in ENVS:
        got = gn_sweep(L, cases) if value is None and clean else _child_sweep(name, value)
        want = [gn_ladder(c, no_wave=name == "DCAMD_GN_NO_WAVE", span_all=name == "DCAMD_GN_SPAN")[0] for c in cases]
        out[name] = (cases, got, want)
    return out


def test_groupnorm_variant_matches_the_ladder_it_replaced():
    tables = _gn_tables()
    ngrid = 2 * 3 * 8 * 9 * 2 * 3 * 2 * 2
    seen = collections.Counter()
    for name, (cases, got, want) in tables.items():
        bad = [i for i in range(len(cases)) if got[i] != want[i]]
        msg = "\n".join(f"{cases[i]}\n  got {got[i]!r} want {want[i]!r}" for i in bad[:10])
        assert not bad, f"{name}: {len(bad)} of {len(cases)} cases leave the ladder's route\n{msg}"
        seen.update(got)
        hist = collections.Counter(want[:ngrid])
        print(name, dict(hist))
        if name == "default":       # the restatement itself, against the counts it gave when it was written from the ladder
            assert hist == dict(wave=368, image=1452, stats=1728, qaffine=816, invalid=5040, **{"stats+apply": 598, "qfold+span": 194, "qfold+apply": 172})
        if name == "DCAMD_GN_NO_WAVE":
            assert "wave" not in hist and hist["image"] == 1820
        if name == "DCAMD_GN_SPAN":
            assert hist["span"] == 156 and hist["image"] == 1296
    for r in GN_ROUTES + ["invalid"]:       # a sweep that stopped reaching a route must not pass quietly
        assert seen[r] > 0, r
    assert set(seen) == set(GN_ROUTES + ["invalid"]), seen


def test_groupnorm_route_does_not_depend_on_n():
    L = _load_lib()
    pairs = gn_grid(L.lib())
    for name, (cases, got, _) in _gn_tables().items():
        for i, (a, b) in enumerate(pairs):
            assert got[2 * i] == got[2 * i + 1], (name, a, got[2 * i], got[2 * i + 1])


def test_groupnorm_refusals_keep_status_and_text():
    L = _load_lib()
    lib = L.lib()
    cases = [c for c in _flat(gn_grid(lib)) + gn_extra(lib)]
    texts = set()
    for c in cases:
        route, rc, text = gn_ladder(c)
        if route != "invalid":
            continue
        p = L.GroupnormParams(**{k: v for k, v in c.items() if v is not None})
        assert lib.dc_groupnorm_variant(p) == b"invalid", c
        got = lib.dc_groupnorm(p, None)       # returns before any launch
        err = lib.dc_last_error().decode()
        assert got == rc and text in err and err.startswith("dc_groupnorm: "), (c, got, rc, err, text)
        texts.add(text)
    for want in ("null pointer", "statistics-only mode needs", "C0=", "groups=", "n/HW/splits", "x1/C1 mismatch", "in/out dtype must match", "qstats needs",
                 " too large", "grid too large", "dtype 7"):
        assert any(want in t for t in texts), (want, texts)


# ---- LayerNorm -----------------------------------------------------------------------------------------------------------------------
def ln_ladder(c):
    dt, C, rows = c["dtype"], c["C"], c["rows"]
    epc = 4 if dt == F32 else 8
    if dt != c["out_dtype"]:
        return "invalid", ERR_DTYPE, "in/out dtype must match"
    if rows <= 0 or C <= 0 or C % epc:
        return "invalid", ERR_SHAPE, f"rows={rows} C={C}"
    if (c["gamma"] is None) != (c["beta"] is None):
        return "invalid", ERR_ARG, "gamma/beta"
    if (c["scale"] is None) != (c["shift"] is None):
        return "invalid", ERR_ARG, "scale/shift"
    if c["scale"] is not None and not (c["rows_per_sample"] > 0 and c["mod_ld"] >= C):
        return "invalid", ERR_SHAPE, "rows_per_sample/mod_ld"
    ptrs = (c["gamma"] or 0) | (c["beta"] or 0) | (c["scale"] or 0) | (c["shift"] or 0)
    vec16 = C // epc <= 128 and ptrs % 16 == 0 and c["mod_ld"] % 4 == 0
    if vec16 and dt != F32 and C // epc <= 96:
        return "ln16x2", OK, ""
    if dt not in (F32, BF16, F16):
        return "invalid", ERR_DTYPE, f"dtype {dt}"
    return ("ln16" if vec16 else "ln"), OK, ""


def ln_case(dt, C, rows, mod, mod_ld, gamma=FAKE, **over):
    c = dict(x=FAKE, y=FAKE, dtype=dt, out_dtype=dt, rows=rows, C=C, rows_per_sample=rows, mod_ld=mod_ld, eps=1e-5, gamma=gamma, beta=FAKE,
             scale=FAKE if mod else None, shift=FAKE if mod else None, mod_map=None)
    c.update(over)
    return c


def test_layernorm_variant_matches_the_ladder_it_replaced():
    L = _load_lib()
    lib = L.lib()
    seen = collections.Counter()
    for dt, C, mod, ld2, gamma in itertools.product((F32, BF16, F16), (64, 68, 256, 512, 768, 1024, 1152, 4096), (False, True), (0, 2), (FAKE, FAKE + 4)):
        names = []
        for rows in (1, 33, 8000):
            c = ln_case(dt, C, rows, mod, C + ld2, gamma)
            want, rc, text = ln_ladder(c)
            p = L.LayernormParams(**{k: v for k, v in c.items() if v is not None})
            got = lib.dc_layernorm_variant(p).decode()
            assert got == want, (c, got, want)
            if want == "invalid":
                assert lib.dc_layernorm(p, None) == rc and text in lib.dc_last_error().decode(), (c, lib.dc_last_error())
            names.append(got)
        assert len(set(names)) == 1, (dt, C, mod, ld2, names)       # a row never depends on the launch's row count
        seen[names[0]] += 1
        # the rules in words: 16-bit rows up to C = 768 two rows per lane group, fp32 up to 512 and 16-bit at 1024 one, the rest by wave
        if C == 68 and dt != F32:
            assert names[0] == "invalid"
        elif ld2 or gamma != FAKE or C > (512 if dt == F32 else 1024):
            assert names[0] == "ln"
        else:
            assert names[0] == ("ln16" if dt == F32 or C == 1024 else "ln16x2")
    assert set(seen) == {"ln16x2", "ln16", "ln", "invalid"}, seen
    b = ln_case(BF16, 2048, 4, True, 2048)
    for over in (dict(x=None), dict(out_dtype=F16), dict(rows=0), dict(beta=None), dict(shift=None), dict(rows_per_sample=0), dict(mod_ld=2040),
                 dict(dtype=7, out_dtype=7)):
        c = dict(b, **over)
        want, rc, text = ("invalid", ERR_ARG, "null pointer") if c["x"] is None else ln_ladder(c)
        p = L.LayernormParams(**{k: v for k, v in c.items() if v is not None})
        assert want == "invalid" and lib.dc_layernorm_variant(p) == b"invalid", c
        assert lib.dc_layernorm(p, None) == rc and text in lib.dc_last_error().decode(), (c, lib.dc_last_error())


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--child":
        L = _load_lib()
        with open(sys.argv[2], "w") as f:
            json.dump(gn_sweep(L, _flat(gn_grid(L.lib())) + gn_extra(L.lib())), f)
