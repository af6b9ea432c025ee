"""The tone inputs of tests/test_gpu_analysis_copies.py pin the oracle's pick on every frame: no exact tie, and a margin to every other
bin of more than twice the FP16 map bar (2e-4 of the map's peak, tests/test_gpu_pair_levels.py's TOL_E) -- so that test compares the
bins of ALL their frames for equality and skips none.  No GPU: the fp64 oracle alone."""
import numpy as np
import pytest

pytest.importorskip("torch")
import test_gpu_analysis_copies as t                           # noqa: E402


@pytest.mark.parametrize("case", list(t.TONE_CASES))
def test_the_oracle_alone_gives_a_unique_pick_on_every_frame_of_the_tone_inputs(case):
    pcm = t._tone_input(case)
    o = t.oracle_picks(pcm[0])
    margin = t.pick_margins(o)
    print("%s: bins %s, smallest margin %.3e of the map's peak" % (case, np.unique(o["bin"]).tolist(), margin.min()))
    assert margin.shape == (2 * t.F1,) and (margin > 2 * 2e-4).all(), margin.tolist()
    assert (np.abs(np.rad2deg(o["doa"][:, 0]) + 33.0) <= 0.5).all()          # ... and it is the source's angle
