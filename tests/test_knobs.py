"""The library's environment knobs have ONE table, lowrankmodels.jl_amd/csrc/glrm_knobs.hpp: the table is well formed, nothing else under
csrc/ spells a knob's name, every GLRM_HIP_* / GLRM_EXCHANGE_* name the tree's tests, tools and documents use is a row of it (a misspelt knob
in a test would silently test the default), and DESIGN.md's table states the same defaults and read times."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lowrankmodels.jl_amd", "csrc")
ROW = re.compile(r'^\s*X\((HIP|EXCHANGE),\s*(\w+),\s*(\w+),\s*([-\w]+),\s*(\w+),\s*(\w+),\s*"((?:[^"\\]|\\.)*)"\)', re.M)
NAME = re.compile(r"GLRM_(?:HIP|EXCHANGE)_[A-Z0-9_]*")

# names that are no row of the table: {name: (reason, the only files that may use it, or None for any)}
ALLOWED = {
    "GLRM_HIP_LIB": ("which library julia/HipGLRM.jl loads: read by the Julia shim, not by the library", None),
    "GLRM_HIP_LIB_PATH": ("which library _capi.py loads (variant builds): read by the Python loader, not by the library", None),
    "GLRM_HIP_CACHED_GRID_PCT": ("a variant build's knob: bench_storage_cached.py describes the one-line variant that reads it", ("tests/perf/bench_storage_cached.py", "DESIGN.md")),
    "GLRM_HIP_BLOCKED_XGATE": ("retired (per-XCD pacing, measured and dropped): the historical mention in the pacing test's docstring", ("tests/test_gpu_blocked_pacing.py",)),
    "GLRM_HIP_ABI_VERSION": ("a macro of include/glrm_hip.h, not an environment variable", None),
    "GLRM_HIP_TESTING": ("the compile-time switch of the test build, not an environment variable", None),
}
# tools/SESSIONS.md is the log of past measurement sessions: it quotes the command lines of variant builds whose switches never shipped
SESSION_LOG_ONLY = {"GLRM_HIP_TILE_STAGGER", "GLRM_HIP_ROW_SPLIT", "GLRM_HIP_TILE_LW", "GLRM_HIP_TILE_LW_SIDES", "GLRM_HIP_UNROLL_LONG",
                    "GLRM_HIP_LANE_CSR_CLASSES", "GLRM_HIP_LANE_TRIAL_WAVES"}
ALLOWED.update({name: ("a variant build's switch quoted in the session log", ("tools/SESSIONS.md",)) for name in SESSION_LOG_ONLY})


def table():
    text = open(os.path.join(CSRC, "glrm_knobs.hpp")).read()
    rows = [dict(zip(("prefix", "suffix", "kind", "default", "read", "build", "doc"), m.groups())) for m in ROW.finditer(text)]
    for r in rows:
        r["name"] = f"GLRM_{r['prefix']}_{r['suffix']}"
    assert len(rows) == len(re.findall(r"^\s*X\((?:HIP|EXCHANGE),", text, re.M)), "a row of the table does not parse"
    return rows


def test_the_table_is_well_formed():
    rows = table()
    assert len(rows) >= 50
    names = [r["name"] for r in rows]
    assert len(set(names)) == len(names), sorted(n for n in names if names.count(n) > 1)
    assert len({r["suffix"] for r in rows}) == len(rows)   # the suffix alone is the enumerator
    for r in rows:
        assert r["kind"] in ("INT", "FLOAT", "PATH") and r["read"] in ("SETUP", "CALL") and r["build"] in ("ANY", "TESTING"), r
        assert r["default"] == "AUTO" or re.fullmatch(r"-?\d+", r["default"]), r
        assert len(r["doc"].strip()) > 20 and r["doc"].rstrip().endswith("."), r
        if r["default"] == "AUTO":
            assert "AUTO" in r["doc"], f"{r['name']}: the meaning of an AUTO row says what the default is computed from"
    testing_only = {r["name"] for r in rows if r["build"] == "TESTING"}
    assert {n for n in names if n.startswith("GLRM_EXCHANGE_EMULATE_")} | {"GLRM_HIP_TEST_FAIL_FINALIZE"} <= testing_only


def test_no_other_file_under_csrc_names_a_knob_or_reads_the_environment():
    bad = []
    for path in sorted(glob.glob(os.path.join(CSRC, "*"))):
        if os.path.basename(path) == "glrm_knobs.hpp":
            continue
        for no, line in enumerate(open(path, errors="replace"), 1):
            if re.search(r'"GLRM_(HIP|EXCHANGE)_', line) or re.search(r"\b(getenv|env_int)\s*\(", line):
                bad.append(f"{os.path.basename(path)}:{no}: {line.strip()[:120]}")
    assert not bad, "\n".join(bad)


def places():
    out = [os.path.join(ROOT, f) for f in ("bench.py", "bench_legs.py", "README.md", "DESIGN.md", "INTEGRATION.md")]
    out += glob.glob(os.path.join(ROOT, "tests", "**", "*.py"), recursive=True)
    for d in ("tools", "julia"):
        out += [p for p in glob.glob(os.path.join(ROOT, d, "**", "*"), recursive=True) if os.path.isfile(p)]
    return sorted(set(out))


def test_every_name_the_tree_uses_is_in_the_table():
    names = {r["name"] for r in table()}
    unknown = []
    for path in places():
        rel = os.path.relpath(path, ROOT)
        if rel == os.path.join("tests", "test_knobs.py"):
            continue
        for no, line in enumerate(open(path, errors="replace"), 1):
            for name in NAME.findall(line):
                if name in names:
                    continue
                if name.endswith("_"):   # a prefix ("GLRM_EXCHANGE_EMULATE_*", a name put together from a prefix and a key)
                    if any(n.startswith(name) for n in names):
                        continue
                elif name in ALLOWED and (ALLOWED[name][1] is None or rel in ALLOWED[name][1]):
                    continue
                unknown.append(f"{rel}:{no}: {name}")
    assert not unknown, "names that are no row of csrc/glrm_knobs.hpp (misspelt, retired, or to be added to ALLOWED with a reason):\n" + "\n".join(unknown)


def test_design_md_states_the_table():
    doc = {}
    for line in open(os.path.join(ROOT, "DESIGN.md")):
        m = re.match(r"\| `(GLRM_(?:HIP|EXCHANGE)_[A-Z0-9_]+)` \| ([^|]*) \| (SETUP|CALL)[^|]* \|", line)
        if m:
            assert m.group(1) not in doc, f"{m.group(1)} has two rows in DESIGN.md"
            doc[m.group(1)] = (m.group(2).strip(), m.group(3))
    rows = table()
    assert set(doc) == {r["name"] for r in rows}, sorted(set(doc) ^ {r["name"] for r in rows})
    for r in rows:
        default, read = doc[r["name"]]
        assert read == r["read"], (r["name"], read, r["read"])
        if r["default"] != "AUTO":
            assert default.replace("`", "") == r["default"], (r["name"], default, r["default"])
        else:
            assert default.startswith("auto"), (r["name"], default)
