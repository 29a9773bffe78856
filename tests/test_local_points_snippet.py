"""CPU: the drop-in body of Tracking::SearchLocalPoints (csrc/adapter/snippets/Tracking_SearchLocalPoints_hip.cc, replacing
Tracking.cc:3449-3539) type-checks against the reference's unmodified Tracking.h / Frame.h / MapPoint.h / LocalMapping.h / Atlas.h.
Third-party headers are declaration-only doubles: tests/support/slam_typecheck_stub/ (the matcher adapter's) behind
tests/support/tracking_typecheck_stub/ (what Tracking.h's include chain adds).  -fsyntax-only, only this repository's file.
Skipped where /root/reference is absent (e.g. on the GPU box)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference"
REF_INC = os.path.join(REF, "include")
SNIPPET = os.path.join(ROOT, "3_orb_slam3_selfnote_amd", "csrc", "adapter", "snippets", "Tracking_SearchLocalPoints_hip.cc")


def _check(path):
    cmd = ["g++", "-std=c++11", "-fsyntax-only", "-I", os.path.join(ROOT, "tests", "support", "tracking_typecheck_stub"),
           "-I", os.path.join(ROOT, "tests", "support", "slam_typecheck_stub"), "-I", REF_INC, "-I", os.path.join(REF_INC, "CameraModels"),
           "-I", REF, "-I", os.path.join(ROOT, "include"), path]
    return subprocess.run(cmd, capture_output=True, text=True)


pytestmark = pytest.mark.skipif(not os.path.exists(os.path.join(REF_INC, "Tracking.h")) or shutil.which("g++") is None,
                                reason="reference headers or g++ not available")


def test_tracking_snippet_typechecks():
    r = _check(SNIPPET)
    assert r.returncode == 0, r.stderr[-4000:]


def test_the_check_sees_a_wrong_member(tmp_path):
    """The doubles do not swallow errors in the snippet itself: a misspelled Frame member is reported."""
    src = open(SNIPPET).read()
    assert "mCurrentFrame.mfLogScaleFactor" in src
    bad = tmp_path / "Tracking_SearchLocalPoints_bad.cc"
    bad.write_text(src.replace("mCurrentFrame.mfLogScaleFactor", "mCurrentFrame.mfLogScaleFactr"))
    r = _check(str(bad))
    assert r.returncode != 0 and "mfLogScaleFactr" in r.stderr
