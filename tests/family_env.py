"""Forcing environments of the GPU tests: the knob settings that put a small problem on one kernel family or one launch form, spelled
once (imported like `cases` and `shapes`).  Names, defaults and meanings: lowrankmodels.jl_amd/csrc/glrm_knobs.hpp -- tests/test_knobs.py
holds every name used under tests/ to that table, so a misspelt knob here fails there instead of silently testing the default."""


def blocked(tps="1", fill="3"):
    """Phase-aligned passes on both views: `tps` LDS-tile units per super-tile (1: many super-tiles -- the partial sums per (segment,
    super-tile) and their fixed-order reduction are exercised) and `fill` percent of the chip's residency per launch slice (3: many
    slices per pass); the cached row sweep off, which would otherwise own the short rows."""
    return {"GLRM_HIP_BLOCKED": "3", "GLRM_HIP_BLOCKED_TPS": tps, "GLRM_HIP_BLOCKED_FILL": fill, "GLRM_HIP_CACHED": "0"}


GATHER = {"GLRM_HIP_CACHED": "0", "GLRM_HIP_BLOCKED": "0"}   # the plain gather sweeps on both views
FOUR_LANE = {"GLRM_HIP_LANE": "0"}                            # LDS tiles at k = 32 on the four-lane kernels, not the lane-per-segment passes


def cached(persist=True):
    """The cached row sweep wherever the rows fit, columns on the gather sweep; persist=False: its one-row-per-workgroup kernel."""
    env = dict(GATHER, GLRM_HIP_CACHED="1")
    if not persist:
        env["GLRM_HIP_CACHED_PERSIST"] = "0"
    return env


# the forms of the lane-per-segment passes (k = 32): stream forms and slot deal (set-up), and each form of the trial rounds forced on
# every round (per call) -- all of them add the same terms in the same order
LANE_FORMS = {
    "default": {},
    "deal off": {"GLRM_HIP_LANE_DEAL": "0"},
    # the COMPACT form of the stream (2-byte offsets padded, values unpadded: what views beyond 2e9 observations run) on every side it serves
    "compact stream": {"GLRM_HIP_LANE_COMPACT": "1"},
    "older forms (full grid / CSR)": {"GLRM_HIP_LANE_ROUNDS": "0"},
    "gathered, chunk lists": {"GLRM_HIP_LANE_GATHER_TO": "101", "GLRM_HIP_LANE_GATHER_PACKED": "0"},
    "gathered, packed lists": {"GLRM_HIP_LANE_GATHER_TO": "101", "GLRM_HIP_LANE_GATHER_PACKED": "101", "GLRM_HIP_LANE_GATHER_SPREAD": "1000"},
    # every round after the first (and a first trial of few rows) on the tail kernel: a wave per (segment, super-tile), no tile
    "a wave per row": {"GLRM_HIP_LANE_TAIL": "101", "GLRM_HIP_LANE_TAIL_COLS": "101"},
    "no tail kernel": {"GLRM_HIP_LANE_TAIL": "0", "GLRM_HIP_LANE_TAIL_COLS": "0"},
}
LANE_FORM_KEYS = tuple(sorted({key for env in LANE_FORMS.values() for key in env}))


def lane_forms(*names):
    return {name: LANE_FORMS[name] for name in names}


def setenv(monkeypatch, env):
    for key, value in env.items():
        monkeypatch.setenv(key, value)
