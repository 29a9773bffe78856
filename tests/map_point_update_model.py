"""numpy model of MapPoint::ComputeDistinctiveDescriptors (MapPoint.cc:350-436) and MapPoint::UpdateNormalAndDepth (MapPoint.cc:467-547)
for the points of tests/map_point_update_scene.py.

UpdateNormalAndDepth is written in np.float32 / np.float64 scalar operations in the order csrc/orb_ref_mappoint.h states:
  normali = mWorldPos - Owi                       float subtraction per component
  cv::norm(v)                                     squares accumulated in double in index order, a double sqrt
  normal = normal + normali/cv::norm(normali)     cv::scaleAdd: alpha = (float)(1.0 / norm), the product rounded to float, then the sum
  dist (const float)                              the double norm rounded once
  mfMaxDistance = dist*scale, mfMinDistance = mfMaxDistance/maxScale     float product, float division
  mNormalVector = normal/n                        (float)((double)v * (1.0 / (double)n))
`form` / `final` select the neighbouring candidates, so that a scene can show that it tells them apart:
  form  "scaleadd" (stated) | "fused" (one rounding of src1*alpha + src2) | "divide" (normali[k] / (float)norm, then the sum)
        | "divide64" ((float)(normali[k] / norm) in double, then the sum)
  final "mul" (stated) | "div" (a plain float x / n)
The descriptor choice goes through the oracle's distinctive_descriptor on the flagged rows, mapped back to entry indices."""
import numpy as np

f32, f64 = np.float32, np.float64


def norm_double(v):
    acc = f64(0.0)
    for k in range(3):
        acc = acc + f64(v[k]) * f64(v[k])
    return np.sqrt(acc)


def normal_depth(centre, pos, ref_centre, ref_scale, ref_max_scale, form="scaleadd", final="mul"):
    """(normal [3], min_dist, max_dist) as float32 for one point with len(centre) >= 1 entries."""
    pos, ref_centre = np.asarray(pos, f32), np.asarray(ref_centre, f32)
    centre = np.asarray(centre, f32).reshape(-1, 3)
    normal = [f32(0.0)] * 3
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        for c in centre:
            d = [f32(pos[k] - c[k]) for k in range(3)]
            n = norm_double(d)
            alpha = f32(f64(1.0) / n)
            for k in range(3):
                if form == "scaleadd":
                    normal[k] = f32(f32(d[k] * alpha) + normal[k])
                elif form == "fused":                                  # exact product and sum in double (24 x 24 bits), rounded once
                    normal[k] = f32(f64(d[k]) * f64(alpha) + f64(normal[k]))
                elif form == "divide":
                    normal[k] = f32(f32(d[k] / f32(n)) + normal[k])
                elif form == "divide64":
                    normal[k] = f32(f32(f64(d[k]) / n) + normal[k])
                else:
                    raise ValueError(form)
        pc = [f32(pos[k] - ref_centre[k]) for k in range(3)]
        dist = f32(norm_double(pc))
        max_dist = f32(dist * f32(ref_scale))
        min_dist = f32(max_dist / f32(ref_max_scale))
        cnt = len(centre)
        if final == "mul":
            out = [f32(f64(normal[k]) * (f64(1.0) / f64(cnt))) for k in range(3)]
        else:
            out = [f32(normal[k] / f32(cnt)) for k in range(3)]
    return np.array(out, f32), min_dist, max_dist


def best_entry(oracle, desc, in_desc):
    """Entry index of the descriptor :389-435 keeps among the flagged rows, -1 where none is flagged."""
    rows = np.nonzero(np.asarray(in_desc) != 0)[0]
    if len(rows) == 0:
        return -1
    return int(rows[oracle.distinctive_descriptor(np.ascontiguousarray(np.asarray(desc, np.uint8)[rows]))])


def update(oracle, points, fill, form="scaleadd", final="mul"):
    """(best, normal, min_dist, max_dist) over all points; a point without entries has best -1 and keeps `fill` in its floats."""
    n = len(points)
    best = np.full(n, -1, np.int32)
    normal, mn, mx = np.full((n, 3), fill, f32), np.full(n, fill, f32), np.full(n, fill, f32)
    for p, pt in enumerate(points):
        if len(pt["desc"]) == 0:
            continue
        if oracle is not None:
            best[p] = best_entry(oracle, pt["desc"], pt["in_desc"])
        normal[p], mn[p], mx[p] = normal_depth(pt["centre"], pt["pos"], pt["ref_centre"], pt["ref_scale"], pt["ref_max_scale"], form, final)
    return best, normal, mn, mx


def same_bits(a, b):
    """Equal NaN masks, and equal bits wherever the value is not a NaN (a NaN's payload and sign are not part of the statement)."""
    a, b = np.asarray(a, f32), np.asarray(b, f32)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb])
