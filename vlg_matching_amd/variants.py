"""Builds of the library with other build-time constants, and runs of the default build with the runtime switches.

The table is shared by __graft_entry__.build(), which compiles every variant out of tree (csrc/Makefile, target `variant`), and by
tests/test_gpu_variants.py, which runs the small-text parity tests once per variant and once per environment run, each in a fresh
process.  Every value here changes compiled code or the path taken: a constant at its default, or a switch another one masks, is left
out."""
import os
import subprocess
from concurrent.futures import ThreadPoolExecutor

_HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(_HERE)
CSRC = os.path.join(_HERE, "csrc")

# the defaults of csrc/ (what vlg_build_constants reports for the in-tree library)
DEFAULTS = {
    "VLG_LINK_RUN": 2048, "VLG_COOP_WINDOWS2": 4, "VLG_RUNG_SHIFT": 2, "VLG_RESOLVE_HOPS": 4096, "VLG_RESOLVE_CHUNK": 4096,
    "VLG_GROUP_CHUNK": 2048, "VLG_STAGE_LISTS": 1, "VLG_SWEEP_PAIRS": 1, "VLG_PIVOT_GROUPS": 2, "VLG_PIVOT_TURNS": 1,
    "VLG_COMPACT_RUNS": 16, "VLG_SPARSE_TURN": 8, "VLG_SORT_CLASSES": 5, "VLG_BUCKET_SORT": 1, "VLG_WINDOW_SORT": 1,
    "VLG_WINDOWS_PER_TILE": 2, "VLG_WINDOW_RANK_LOOP": 0, "VLG_WINDOW_THREADS": 256, "VLG_WINDOW_ITEMS": 12, "VLG_FETCH_THREADS": 16,
    "VLG_DOCLIST_RUN": 2048, "VLG_SWEEP_CHUNK": 2048, "VLG_LINK_EARLY": 1, "VLG_ONE_PASS_MAX": 131072,
}

VARIANTS = {
    # every size constant at or near its smallest legal value: the small test texts cross each tile, run and chunk border hundreds
    # of times, and chains of trail records outlast a resolve round.  (VLG_LINK_RUN = 3 x 64, not 64: a run then holds one two-step
    # pair and one single step, so both paths of the link pass run and every run ends inside a 128-key step.  VLG_DOCLIST_RUN = 192:
    # three steps per run of the document listing, so a block of four runs ends off every power of two.  VLG_SWEEP_CHUNK = 512: two
    # rows per turn of a sweep round -- the fewest that pairs of rows allow -- so the survivors' look-back links hundreds of turns.
    # VLG_ONE_PASS_MAX = 8192: the long lists of the small texts fall on both sides of the one-pass bound of the sort.)
    "small": {"VLG_LINK_RUN": 192, "VLG_RESOLVE_CHUNK": 256, "VLG_GROUP_CHUNK": 256, "VLG_RESOLVE_HOPS": 2, "VLG_COMPACT_RUNS": 1,
              "VLG_SPARSE_TURN": 1, "VLG_PIVOT_GROUPS": 1, "VLG_COOP_WINDOWS2": 1, "VLG_DOCLIST_RUN": 192, "VLG_SWEEP_CHUNK": 512, "VLG_ONE_PASS_MAX": 8192},
    # the kept build-time alternates on their other side; VLG_RUNG_SHIFT 4 does not divide 6, so the fences are built apart from the rungs;
    # VLG_LINK_EARLY 0: the pair search of the link pass loads a window when it turns to it; VLG_ONE_PASS_MAX 0: no one-pass lists in the sort
    "alternates": {"VLG_SORT_CLASSES": 3, "VLG_SWEEP_PAIRS": 0, "VLG_STAGE_LISTS": 0, "VLG_WINDOW_RANK_LOOP": 1, "VLG_WINDOWS_PER_TILE": 4,
                   "VLG_PIVOT_TURNS": 4, "VLG_RUNG_SHIFT": 4, "VLG_LINK_EARLY": 0, "VLG_ONE_PASS_MAX": 0},
    # block-wide radix sorts instead of the bucket sorts (VLG_BUCKET_SORT=0 makes VLG_WINDOW_RANK_LOOP moot, hence a variant of its
    # own), and a ladder of fan 8 whose second level is the fences
    "radix": {"VLG_BUCKET_SORT": 0, "VLG_RUNG_SHIFT": 3},
}

# a run of the default library with the runtime switches that select a second path (none of them masks another)
ENV_RUNS = {
    "env_paths": {"VLG_RESOLVE_GROUPED": "0", "VLG_SWEEP_LOOKAHEAD": "0", "VLG_NO_SPECULATIVE_COMPACT": "1", "VLG_WINDOW_SORT": "0",
                  "VLG_FUSE_JUMP": "0"},
}


def constants(name):
    """The constants variant `name` is compiled with (None: the in-tree default build)."""
    c = dict(DEFAULTS)
    if name is not None:
        c.update(VARIANTS[name])
    return c


def extra_defs(name):
    return " ".join("-D%s=%d" % kv for kv in sorted(VARIANTS[name].items()))


def library(name):
    return os.path.join(ROOT, "build", "variants", name, "libvlg_hip.so")


def build(name, jobs=4):
    subprocess.check_call(["make", "-C", CSRC, "-j%d" % jobs, "variant", "VARIANT=" + name, "EXTRA_DEFS=" + extra_defs(name)],
                          stdout=subprocess.DEVNULL)


def build_all(jobs=None):
    """Every variant, side by side (each is a few minutes of hipcc on one core per object)."""
    jobs = jobs or max(1, min(8, (os.cpu_count() or 4) // len(VARIANTS)))
    with ThreadPoolExecutor(len(VARIANTS)) as ex:
        for f in [ex.submit(build, n, jobs) for n in VARIANTS]:
            f.result()
