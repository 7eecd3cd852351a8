"""Every flagged frame through every host path, word for word: the 22 legal combinations of RTG_FLAG_SUM_SQUARES, SAMPLE_COUNTS,
RETIRE, DENOISE, FEATURES and DENOISE_ERROR on a 23 x 17 frame (every even-word rounding of the layout bites), whole and as a
PARTIAL then a RESUME slice, through rtg_par_cast, rtg_par_cast_device and rtg_par_cast_multi, on the lean pool, the full-feature
/ lock-step and the baseline kernels.  The SHA-256 of the whole frame after each call must be the one recorded in
tests/golden/flag_frame_digests.json -- by tools/gen_flag_frame_digests.py on an MI355X, from the commit BEFORE the host launcher
was given one frame layout, one post-step order and one variant pick; a combination that commit refuses must be refused alike."""
import json
import os

import pytest

import flag_frames

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "flag_frame_digests.json")


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as fh:
        return json.load(fh)


@pytest.mark.parametrize("path", flag_frames.PATHS)
@pytest.mark.parametrize("setup", list(flag_frames.SETUPS))
def test_frames_are_the_recorded_ones(pkg, gpu, golden, setup, path):
    want = golden["%s/%s" % (setup, path)]
    assert len(flag_frames.COMBOS) == 22 and len(want) == 2 * 22
    got = flag_frames.digests(pkg, gpu, setup, path)
    assert sorted(got) == sorted(want)
    bad = {k: (got[k], want[k]) for k in want if got[k] != want[k]}
    assert not bad, "%d of %d frames differ from the recorded ones: %s" % (len(bad), len(want), sorted(bad)[:8])
    assert any(not d.startswith("error") for v in got.values() for d in v)   # (the case renders)
