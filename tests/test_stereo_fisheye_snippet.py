"""CPU: the drop-in body of Frame::ComputeStereoFishEyeMatches (csrc/adapter/snippets/Frame_ComputeStereoFishEyeMatches_hip.cc,
replacing Frame.cc:1228-1268) type-checks against the reference's unmodified Frame.h and GeometricCamera.h.  Third-party headers
are the declaration-only doubles of tests/support/ that tests/test_local_points_snippet.py uses.  -fsyntax-only, only this
repository's file.  Skipped where the reference tree is absent."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference"
REF_INC = os.path.join(REF, "include")
SNIPPET = os.path.join(ROOT, "3_orb_slam3_selfnote_amd", "csrc", "adapter", "snippets", "Frame_ComputeStereoFishEyeMatches_hip.cc")


def _check(path):
    cmd = ["g++", "-std=c++11", "-fsyntax-only", "-I", os.path.join(ROOT, "tests", "support", "tracking_typecheck_stub"),
           "-I", os.path.join(ROOT, "tests", "support", "slam_typecheck_stub"), "-I", REF_INC, "-I", os.path.join(REF_INC, "CameraModels"),
           "-I", REF, "-I", os.path.join(ROOT, "include"), path]
    return subprocess.run(cmd, capture_output=True, text=True)


pytestmark = pytest.mark.skipif(not os.path.exists(os.path.join(REF_INC, "Frame.h")) or shutil.which("g++") is None,
                                reason="reference headers or g++ not available")


def test_snippet_typechecks():
    r = _check(SNIPPET)
    assert r.returncode == 0, r.stderr[-4000:]


def test_the_check_sees_a_wrong_member(tmp_path):
    """The doubles do not swallow errors in the snippet itself: a misspelled Frame member is reported."""
    src = open(SNIPPET).read()
    assert "mvRightToLeftMatch.data()" in src
    bad = tmp_path / "Frame_ComputeStereoFishEyeMatches_bad.cc"
    bad.write_text(src.replace("mvRightToLeftMatch.data()", "mvRightToLeftMatchs.data()"))
    r = _check(str(bad))
    assert r.returncode != 0 and "mvRightToLeftMatchs" in r.stderr
