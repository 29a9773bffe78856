"""CPU: the two adapter snippets of the local-map entries type-check against the reference's own headers (g++ -fsyntax-only with the stub
directories of tests/support), the check sees a wrong member, and each snippet states its edits and its notes."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference"
REF_INC = os.path.join(REF, "include")
SNIPPETS = os.path.join(ROOT, "3_orb_slam3_selfnote_amd", "csrc", "adapter", "snippets")
TRACKING = os.path.join(SNIPPETS, "Tracking_UpdateLocalMap_hip.cc")
KEYFRAME = os.path.join(SNIPPETS, "KeyFrame_UpdateConnections_hip.cc")
needs_reference = pytest.mark.skipif(not os.path.exists(os.path.join(REF_INC, "Tracking.h")) or shutil.which("g++") is None,
                                     reason="reference headers or g++ not available")


def _typecheck(path):
    """The command of tests/test_keyframe_culling_abi.py."""
    cmd = ["g++", "-std=c++11", "-fsyntax-only", "-I", os.path.join(ROOT, "tests", "support", "tracking_typecheck_stub"),
           "-I", os.path.join(ROOT, "tests", "support", "slam_typecheck_stub"), "-I", REF_INC, "-I", os.path.join(REF_INC, "CameraModels"),
           "-I", REF, "-I", os.path.join(ROOT, "include"), path]
    return subprocess.run(cmd, capture_output=True, text=True)


@needs_reference
@pytest.mark.parametrize("path", [TRACKING, KEYFRAME])
def test_snippet_typechecks(path):
    r = _typecheck(path)
    assert r.returncode == 0, r.stderr[-4000:]


@needs_reference
@pytest.mark.parametrize("path,member", [(TRACKING, "GetBestCovisibilityKeyFrames"), (TRACKING, "mnTrackReferenceForFrame"), (TRACKING, "mpLastKeyFrame"),
                                         (TRACKING, "orbm_update_local_map"), (KEYFRAME, "mConnectedKeyFrameWeights"), (KEYFRAME, "mbFirstConnection"),
                                         (KEYFRAME, "GetInitKFid"), (KEYFRAME, "orbm_update_connections")])
def test_the_check_sees_a_wrong_member(tmp_path, path, member):
    src = open(path).read()
    assert member in src
    bad = tmp_path / os.path.basename(path).replace("_hip", "_bad")
    bad.write_text(src.replace(member, member[:-1] + "z"))
    r = _typecheck(str(bad))
    assert r.returncode != 0 and member[:-1] + "z" in r.stderr, r.stderr[-2000:]


def test_snippets_hold_their_edits_and_notes():
    src = open(TRACKING).read()
    for line in ("void Tracking::UpdateLocalKeyFrames()", "void Tracking::UpdateLocalPoints()", "THE SNAPSHOT", "RANK RULE", "STAMP NOTE",
                 "F.mvpMapPoints[i] = NULL;", "mpReferenceKF = T.kfs[kfMax];", "pMP->mnTrackReferenceForFrame = mCurrentFrame.mnId;"):
        assert line in src, line
    src = open(KEYFRAME).read()
    for line in ("KeyFrameConnections conn(vpKeyFrames);", "conn.apply(pKFi);", "THE SNAPSHOT", "CONNECTIONS RULE", "RANK RULE", "AddConnection(pKF, mConnW[i])",
                 "ordered.front()->AddChild(pKF);"):
        assert line in src, line
    for doc, words in (("INTEGRATION.md", ("Tracking_UpdateLocalMap_hip.cc", "KeyFrame_UpdateConnections_hip.cc")),
                       ("SNIPPETS.md", ("Tracking_UpdateLocalMap_hip.cc", "KeyFrame_UpdateConnections_hip.cc"))):
        text = open(os.path.join(ROOT, doc)).read()
        for w in words:
            assert w in text, (doc, w)
