"""A new context starts from the environment (include/bvc.h, "tuning"): the variables are read through the same table of knobs that
bvc_set_tuning reads, so a process started with them computes what a context given the same values by key computes."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.sitegen import random_site
from tests.test_gpu_parity import pad_rows

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# key: (lowest value, highest value) of include/bvc.h; "em_wpb" takes its two ends only
KNOBS = {"em_waves_per_cu": (0, 32), "em_wpb": (1, 4), "hist_split": (0, 64), "group_pipe": (0, 1), "group_copies_log2": (-1, 5),
         "group_big_lds": (0, 1), "group_h16": (0, 1), "em_streams": (0, 3), "em_engine": (0, 1), "em_tiny_regions": (0, 1),
         "em_prune": (0, 1), "bgzf_codes": (0, 1), "bgzf_parse": (0, 1), "bgzf_cuts": (0, 1), "csr_scatter_max": (0, 1 << 30),
         "stats_copies_log2": (0, 4), "host_chunk_kib": (1, 1 << 21)}

CHILD = """
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
from basevarc_amd import Context
d = np.load(sys.argv[2])
with Context(0) as c:
    np.save(sys.argv[3], c.lrt_dense(d["B"], d["Q"], d["R"], float(d["m"])))
"""


def env_sites(seed=4400, n_sites=60):
    """The sites of test_the_subset_a_level_does_not_run_never_changes_a_record (tests/test_gpu_round4.py), fewer and at most 3000 deep:
    monomorphic, bi- and tri-allelic, two alleles of equal depth."""
    rng = np.random.default_rng(seed)
    sites = []
    for s in range(n_sites):
        nind = int(rng.choice([1, 2, 3, 4, 6, 9, 14, 25, 60, 400, 3000]))
        af = float(rng.choice([0.0, 0.0, 0.01, 0.1, 0.5]))
        b, q, r = random_site(rng, nind, af=af, second_af=(af / 2 if s % 5 == 0 else 0.0))
        if s % 7 == 0 and nind >= 2:                              # two alleles of exactly equal depth, nothing else
            b = np.array([0, 1] * (nind // 2), dtype=np.int8)
            q = q[:len(b)]
        sites.append((b, q, r))
    return sites


def test_a_context_starts_from_the_environment(tmp_path):
    """A fresh process with BVC_EM_PRUNE=0, BVC_EM_WPB=1, BVC_HIST_SPLIT=5 and BVC_GROUP_LOG2C=9 (out of range: the default stays)
    returns the bytes of a context given em_prune 0, em_wpb 1, hist_split 5 by key, and its n_fits differ from an untouched
    context's: the subsets em_prune = 1 does not run (on these sites the oracle's n_fits and n_fits_pruned differ on 6 of the 60).
    Every key takes both ends of its range and refuses the values one beyond them."""
    from basevarc_amd import BvcError, Context
    B, Q, R = pad_rows(env_sites())
    m = 0.001
    np.savez(tmp_path / "sites.npz", B=B, Q=Q, R=R, m=m)
    env = dict(os.environ, BVC_EM_PRUNE="0", BVC_EM_WPB="1", BVC_HIST_SPLIT="5", BVC_GROUP_LOG2C="9")
    subprocess.run([sys.executable, "-c", CHILD, ROOT, str(tmp_path / "sites.npz"), str(tmp_path / "records.npy")], env=env, check=True,
                   timeout=120)
    from_env = np.load(tmp_path / "records.npy")
    with Context(0) as by_key, Context(0) as untouched:
        for key, value in (("em_prune", 0), ("em_wpb", 1), ("hist_split", 5)):
            by_key.set_tuning(key, value)
        assert from_env.tobytes() == by_key.lrt_dense(B, Q, R, m).tobytes()
        assert (from_env["n_fits"] != untouched.lrt_dense(B, Q, R, m)["n_fits"]).any()
        for key, (lo, hi) in KNOBS.items():
            for value in (lo, hi):
                untouched.set_tuning(key, value)
            for value in (lo - 1, hi + 1):
                with pytest.raises(BvcError):
                    untouched.set_tuning(key, value)
