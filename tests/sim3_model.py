"""A literal model of Sim3Solver (Sim3Solver.cc:35-530): the constructor, SetRansacParameters, both overloads of iterate, ComputeCentroid,
ComputeSim3, CheckInliers, Project and FromCameraToImage, written after the reference's text with real loops for the sequential parts, and
of the two OpenCV routines it calls that the project had no statement of: cv::eigen (the two-sided Jacobi for float) and cv::Rodrigues.
It shares no code with the product.

Numbers as in tests/twoview_model.py: a C `double` is a Python float; a C `float` is a Python float that holds a float32 value, and every
float operation is the double operation rounded once more by f32().  libm in double is Python's math module (the same glibc the host form
calls); the float libm calls of KannalaBrandt8::project go through ctypes (tests/rig_stereo_model.py).

The cv::Mat expressions are folded as DESIGN.md section 2 says; each function names its row."""
import math

import numpy as np

import new_points_model as NP
from twoview_model import F, FLT_EPSILON, INF, NAN, ddiv, dsqrt, f32, fadd, fdiv, fmul, fsqrt, fsub, mul_Bt, mul_small

DBL_EPSILON = 2.220446049250313e-16
INT_MIN = -2 ** 31


# ---- libm in double, total (Python raises where C returns NaN or an infinity) ---------------------------------------------------------------
def dlog(x):
    if x != x or x < 0.0:
        return NAN
    if x == 0.0:
        return -INF
    if x == INF:
        return INF
    return math.log(x)


def dpow3(x):
    """pow(x, 3.0)"""
    if x != x:
        return NAN
    try:
        return math.pow(x, 3.0)
    except OverflowError:
        return math.copysign(INF, x)


def dsincos(x):
    if x != x or abs(x) == INF:
        return NAN, NAN
    return math.sin(x), math.cos(x)


def cvtt_f64_i32(x):
    """(int) of a double as x86 converts it (cvttsd2si)"""
    if x != x or x >= 2147483648.0 or x < -2147483648.0:
        return INT_MIN
    return int(x)


def dceil(x):
    if x != x or abs(x) == INF:
        return x
    return float(math.ceil(x))


# ---- SetRansacParameters, :150-174 -------------------------------------------------------------------------------------------------------
def ransac_iterations(probability, min_inliers, max_its, N):
    epsilon = fdiv(f32(min_inliers), f32(N))                                     # (float)mRansacMinInliers/N :161
    if min_inliers == N:
        n = 1                                                                    # :166
    else:
        n = cvtt_f64_i32(dceil(ddiv(dlog(1 - probability), dlog(1 - dpow3(epsilon)))))   # :169
    return max(1, min(n, max_its))                                               # :171


# ---- the constructor, :35-148 --------------------------------------------------------------------------------------------------------------
def transform(T, X):
    """Rcw*X+tcw for a 4 x 4 T (:129, :132, :506): the float sum of products, the addition in double (mat3_mul_add)"""
    return [f32(fadd(fadd(fmul(T[i][0], X[0]), fmul(T[i][1], X[1])), fmul(T[i][2], X[2])) + T[i][3]) for i in range(3)]


def project(cam_type, cam, X):
    """projectMat(cv::Point3f(x, y, z)) (:512, :528)"""
    if cam_type == 0:                                                            # Pinhole.cpp:46-49; z = 0 divides
        p = [float(v) for v in cam]
        return [fadd(fdiv(fmul(p[0], X[0]), X[2]), p[2]), fadd(fdiv(fmul(p[1], X[1]), X[2]), p[3])]
    return list(NP.project(cam_type, cam, X[0], X[1], X[2]))


def max_error(sigma2):
    """mvnMaxError.push_back(9.210*sigmaSquare) into a vector<size_t> (:119-120), then the float it is compared as (:470)"""
    return f32(int(9.210 * float(sigma2)))


def rows44(T):
    return [[float(v) for v in row] for row in np.asarray(T, F).reshape(4, 4)]


class Solver:
    """The members the constructor fills, from the flat problem (the filtering of :85-110 is the caller's, it is not arithmetic)."""

    def __init__(self, prob):
        self.n1 = int(prob["n1"])
        self.idx1 = [int(v) for v in prob["idx1"]]
        self.N = len(self.idx1)
        self.cam1, self.cam2 = (int(prob["cam_type1"]), np.asarray(prob["cam_params1"], F)), (int(prob["cam_type2"]), np.asarray(prob["cam_params2"], F))
        self.fix_scale, self.min_inliers = bool(prob["fix_scale"]), int(prob["min_inliers"])
        self.max_its, self.nIterations = int(prob.get("max_iterations", 300)), int(prob.get("iterations_done", 0))
        T1, T2 = rows44(prob["Tcw1"]), rows44(prob["Tcw2"])
        Xw1, Xw2 = np.asarray(prob["Xw1"], F).reshape(-1, 3), np.asarray(prob["Xw2"], F).reshape(-1, 3)
        self.X1 = [transform(T1, [float(v) for v in Xw1[i]]) for i in range(self.N)]      # mvX3Dc1 :129
        self.X2 = [transform(T2, [float(v) for v in Xw2[i]]) for i in range(self.N)]      # mvX3Dc2 :132, pKF2's pose for every pair
        self.th1 = [max_error(v) for v in np.asarray(prob["sigma2_1"], F).reshape(-1)]    # :119
        self.th2 = [max_error(v) for v in np.asarray(prob["sigma2_2"], F).reshape(-1)]    # :120
        self.im1 = [project(self.cam1[0], self.cam1[1], X) for X in self.X1]              # :143
        self.im2 = [project(self.cam2[0], self.cam2[1], X) for X in self.X2]              # :144
        self.best_inliers, self.best = 0, None


# ---- cv::eigen for a symmetric float matrix ---------------------------------------------------------------------------------------------------
def hypot(a, b):
    """lapack.cpp's own hypot<float>: every step a float operation"""
    a, b = abs(a), abs(b)
    if a > b:
        b = fdiv(b, a)
        return fmul(a, fsqrt(fadd(1.0, fmul(b, b))))
    if b > 0:
        a = fdiv(a, b)
        return fmul(b, fsqrt(fadd(1.0, fmul(a, a))))
    return 0.0


def eigen(A0, info=None):
    """JacobiImpl_<float>: A0 an n x n symmetric float32 matrix.  Returns (W descending, V with the eigenvectors in rows)."""
    n = len(A0)
    A = [[float(v) for v in row] for row in A0]
    V = [[1.0 if i == j else 0.0 for j in range(n)] for i in range(n)]
    W = [A[k][k] for k in range(n)]
    indR, indC = [0] * n, [0] * n

    def row_max(k):
        m, mv = k + 1, abs(A[k][k + 1])
        for i in range(k + 2, n):
            if mv < abs(A[k][i]):
                mv, m = abs(A[k][i]), i
        return m

    def col_max(k):
        m, mv = 0, abs(A[0][k])
        for i in range(1, k):
            if mv < abs(A[i][k]):
                mv, m = abs(A[i][k]), i
        return m

    for k in range(n):
        if k < n - 1:
            indR[k] = row_max(k)
        if k > 0:
            indC[k] = col_max(k)
    iters = 0
    if n > 1:
        while iters < n * n * 30:
            k, mv = 0, abs(A[0][indR[0]])
            for i in range(1, n - 1):
                if mv < abs(A[i][indR[i]]):
                    mv, k = abs(A[i][indR[i]]), i
            l = indR[k]
            for i in range(1, n):
                if mv < abs(A[indC[i]][i]):
                    mv, k, l = abs(A[indC[i]][i]), indC[i], i
            p = A[k][l]
            if abs(p) <= FLT_EPSILON:
                break
            y = f32(fsub(W[l], W[k]) * 0.5)
            t = fadd(abs(y), hypot(p, y))
            s = hypot(p, t)
            c = fdiv(t, s)
            s = fdiv(p, s)
            t = fmul(fdiv(p, t), p)
            if y < 0:
                s, t = -s, -t
            A[k][l] = 0.0
            W[k] = fsub(W[k], t)
            W[l] = fadd(W[l], t)

            def rotate(a0, b0):
                return fsub(fmul(a0, c), fmul(b0, s)), fadd(fmul(a0, s), fmul(b0, c))

            for i in range(k):
                A[i][k], A[i][l] = rotate(A[i][k], A[i][l])
            for i in range(k + 1, l):
                A[k][i], A[i][l] = rotate(A[k][i], A[i][l])
            for i in range(l + 1, n):
                A[k][i], A[l][i] = rotate(A[k][i], A[l][i])
            for i in range(n):
                V[k][i], V[l][i] = rotate(V[k][i], V[l][i])
            for idx in (k, l):
                if idx < n - 1:
                    indR[idx] = row_max(idx)
                if idx > 0:
                    indC[idx] = col_max(idx)
            iters += 1
    for k in range(n - 1):
        m = k
        for i in range(k + 1, n):
            if W[m] < W[i]:
                m = i
        if k != m:
            W[m], W[k] = W[k], W[m]
            V[m], V[k] = V[k], V[m]
    if info is not None:
        info["rotations"] = iters
        info["residual_offdiag"] = max(abs(A[i][j]) for i in range(n) for j in range(i + 1, n))
    return W, V


# ---- cv::Rodrigues, vector to matrix ---------------------------------------------------------------------------------------------------------
def rodrigues(v):
    """A CV_32F 3-vector in, a CV_32F 3 x 3 matrix out, double in between."""
    rx, ry, rz = float(v[0]), float(v[1]), float(v[2])
    theta = dsqrt(rx * rx + ry * ry + rz * rz)
    if theta < DBL_EPSILON:
        return [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]
    s, c = dsincos(theta)
    c1 = 1.0 - c
    itheta = ddiv(1.0, theta) if theta else 0.0
    rx, ry, rz = rx * itheta, ry * itheta, rz * itheta
    rrt = [rx * rx, rx * ry, rx * rz, rx * ry, ry * ry, ry * rz, rx * rz, ry * rz, rz * rz]
    r_x = [0.0, -rz, ry, rz, 0.0, -rx, -ry, rx, 0.0]
    eye = [1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0]
    R = [f32(c * eye[k] + c1 * rrt[k] + s * r_x[k]) for k in range(9)]
    return [R[0:3], R[3:6], R[6:9]]


# ---- ComputeCentroid and ComputeSim3, :329-451 ---------------------------------------------------------------------------------------------
def compute_centroid(P):
    """P: 3 x 3, the points in columns.  Returns (Pr, C)."""
    C = []
    for r in range(3):
        a0, a1 = P[r][0], P[r][1]
        a0 = fadd(a0, P[r][2])
        a0 = fadd(a0, a1)                                   # cv::reduce(P,C,1,CV_REDUCE_SUM) :331
        C.append(f32(a0 * (1.0 / 3.0)))                     # C = C/P.cols :332
    return [[fsub(P[r][c], C[r]) for c in range(3)] for r in range(3)], C


def compute_sim3(P1, P2, fix_scale, info=None):
    """Returns dict(R, t, s, T12, T21, q): mR12i, mt12i, ms12i, mT12i, mT21i and evec.row(0)."""
    Pr1, O1 = compute_centroid(P1)
    Pr2, O2 = compute_centroid(P2)
    M = mul_Bt(Pr2, Pr1)                                    # :357
    N11 = fadd(fadd(M[0][0], M[1][1]), M[2][2])
    N12 = fsub(M[1][2], M[2][1])
    N13 = fsub(M[2][0], M[0][2])
    N14 = fsub(M[0][1], M[1][0])
    N22 = fsub(fsub(M[0][0], M[1][1]), M[2][2])
    N23 = fadd(M[0][1], M[1][0])
    N24 = fadd(M[2][0], M[0][2])
    N33 = fsub(fadd(-M[0][0], M[1][1]), M[2][2])
    N34 = fadd(M[1][2], M[2][1])
    N44 = fadd(fsub(-M[0][0], M[1][1]), M[2][2])
    Nm = [[N11, N12, N13, N14], [N12, N22, N23, N24], [N13, N23, N33, N34], [N14, N24, N34, N44]]
    W, V = eigen(Nm, info)                                  # :386
    if info is not None:
        info["N"], info["eval"], info["evec"] = Nm, W, V
    q = V[0]
    vec = q[1:4]                                            # :389
    nrm = dsqrt(vec[0] * vec[0] + vec[1] * vec[1] + vec[2] * vec[2])
    ang = math.atan2(nrm, q[0])                             # :392
    alpha = (2 * ang) * ddiv(1.0, nrm)
    aa = [f32(v * alpha) for v in vec]                      # :394
    if info is not None:
        info["angle_axis"] = aa
    R = rodrigues(aa)                                       # :398
    P3 = mul_small(R, Pr2)                                  # :402
    if not fix_scale:
        nom = 0.0
        for i in range(3):
            for j in range(3):
                nom += Pr1[i][j] * P3[i][j]                 # Pr1.dot(P3) :408
        den = 0.0
        for i in range(3):
            for j in range(3):
                den += fmul(P3[i][j], P3[i][j])             # :411-420
        s = f32(ddiv(nom, den))                             # :422
    else:
        s = 1.0
    t = []
    for i in range(3):                                      # mt12i = O1 - ms12i*mR12i*O2 :430: one gemm, alpha = -s, beta = 1
        t0 = fadd(fadd(fmul(R[i][0], O2[0]), fmul(R[i][1], O2[1])), fmul(R[i][2], O2[2]))
        t.append(f32(t0 * (-s) + O1[i] * 1.0))
    inv = ddiv(1.0, s)
    sR = [[f32(R[i][j] * s) for j in range(3)] for i in range(3)]           # :437
    sRinv = [[f32(R[j][i] * inv) for j in range(3)] for i in range(3)]      # :446
    tinv = []
    for i in range(3):                                      # -sRinv*mt12i :449
        t0 = fadd(fadd(fmul(sRinv[i][0], t[0]), fmul(sRinv[i][1], t[1])), fmul(sRinv[i][2], t[2]))
        tinv.append(f32(t0 * -1.0 + 0.0))
    T12 = [sR[i] + [t[i]] for i in range(3)] + [[0.0, 0.0, 0.0, 1.0]]
    T21 = [sRinv[i] + [tinv[i]] for i in range(3)] + [[0.0, 0.0, 0.0, 1.0]]
    return dict(R=R, t=t, s=s, T12=T12, T21=T21, q=q)


def hypothesis(S, set3, info=None):
    """The set's columns (:208-209), then ComputeSim3"""
    P1 = [[S.X1[idx][r] for idx in set3] for r in range(3)]
    P2 = [[S.X2[idx][r] for idx in set3] for r in range(3)]
    return compute_sim3(P1, P2, S.fix_scale, info)


# ---- Project and CheckInliers, :454-514 ------------------------------------------------------------------------------------------------------
def dist_dot(a, b):
    dx, dy = fsub(a[0], b[0]), fsub(a[1], b[1])
    d = 0.0
    d += dx * dx
    d += dy * dy
    return f32(d)


def check_pair(S, T12, T21, i):
    """(err1, err2, inlier) of pair i"""
    p2im1 = project(S.cam1[0], S.cam1[1], transform(T12, S.X2[i]))          # :457
    p1im2 = project(S.cam2[0], S.cam2[1], transform(T21, S.X1[i]))          # :458
    err1 = dist_dot(S.im1[i], p2im1)                                         # :464, :467
    err2 = dist_dot(p1im2, S.im2[i])                                         # :465, :468
    return err1, err2, bool(err1 < S.th1[i] and err2 < S.th2[i])


def check_inliers_loop(S, T12, T21):
    mask = [check_pair(S, T12, T21, i)[2] for i in range(S.N)]
    return sum(mask), mask


def _transform_rows(T, X):
    """transform() for all pairs at once: numpy float32 element-wise operations are the same IEEE single operations"""
    T = np.asarray(T, F)
    out = []
    for i in range(3):
        t0 = (T[i, 0] * X[:, 0] + T[i, 1] * X[:, 1]) + T[i, 2] * X[:, 2]
        out.append((t0.astype(np.float64) + np.float64(T[i, 3])).astype(F))
    return out


def _pinhole_rows(cam, X):
    return cam[0] * X[0] / X[2] + cam[2], cam[1] * X[1] / X[2] + cam[3]


def _dist_dot_rows(ax, ay, bx, by):
    dx, dy = (ax - bx).astype(np.float64), (ay - by).astype(np.float64)
    return ((0.0 + dx * dx) + dy * dy).astype(F)


def check_inliers_rows(S, T12, T21):
    """check_pair for all pairs at once, Pinhole cameras only (the large scenes); equal to the loop, which the CPU suite asserts"""
    assert S.cam1[0] == 0 and S.cam2[0] == 0
    with np.errstate(all="ignore"):
        X1, X2, im1, im2 = np.array(S.X1, F), np.array(S.X2, F), np.array(S.im1, F), np.array(S.im2, F)
        u21, v21 = _pinhole_rows(S.cam1[1], _transform_rows(T12, X2))
        u12, v12 = _pinhole_rows(S.cam2[1], _transform_rows(T21, X1))
        err1 = _dist_dot_rows(im1[:, 0], im1[:, 1], u21, v21)
        err2 = _dist_dot_rows(u12, v12, im2[:, 0], im2[:, 1])
        mask = (err1 < np.array(S.th1, F)) & (err2 < np.array(S.th2, F))
    return int(mask.sum()), [bool(v) for v in mask]


def check_inliers(S, T12, T21):
    if S.cam1[0] == 0 and S.cam2[0] == 0 and S.N > 100:
        return check_inliers_rows(S, T12, T21)
    return check_inliers_loop(S, T12, T21)


# ---- iterate, :176-321 ------------------------------------------------------------------------------------------------------------------------
def iterate(S, nIterations, sets, evaluate):
    """Both overloads in one: the loop of :194-237 / :267-315 over this call's sets.  evaluate(k) -> (count, payload) stands for ComputeSim3
    and CheckInliers of the k-th set of the call.  State carried in S: nIterations (mnIterations), best_inliers, best (the payload).
    Returns dict(converged, it_stop, best_it, improved, no_more)."""
    out = dict(converged=0, it_stop=0, best_it=-1, improved=0, no_more=0)
    if S.N < S.min_inliers:                                  # :182, :252
        out["no_more"] = 1
        return out
    cur = 0
    while S.nIterations < S.max_its and cur < nIterations:
        cur += 1
        S.nIterations += 1
        count, payload = evaluate(cur - 1)
        if count >= S.best_inliers:                          # :219, :292
            S.best_inliers, S.best = count, payload
            out["best_it"], out["improved"] = cur - 1, 1     # bestSim3 = mBestT12 :312
            if count > S.min_inliers:                        # :228, :301
                out["converged"], out["it_stop"] = 1, cur
                return out
    out["it_stop"] = cur
    if S.nIterations >= S.max_its:                           # :239, :317
        out["no_more"] = 1
    return out


def ordered_pass(counts, best_in, min_inliers, done, max_its):
    """The SIM3 RULE's one pass over independent counts, written without the loop: the running best in front of every iteration, the
    iterations that reach it, the first of them above min_inliers."""
    counts = np.asarray(counts, np.int64)
    limit = max(0, min(len(counts), max_its - done))
    c = counts[:limit]
    before = np.maximum.accumulate(np.concatenate([[best_in], c]))[:-1] if limit else np.zeros(0, np.int64)
    reach = c >= before
    conv = np.flatnonzero(reach & (c > min_inliers))
    converged = len(conv) > 0
    it_stop = int(conv[0]) + 1 if converged else limit
    reached = np.flatnonzero(reach[:it_stop])
    best_it = int(reached[-1]) if len(reached) else -1
    return dict(converged=int(converged), it_stop=it_stop, best_it=best_it, improved=int(best_it >= 0),
                best_inliers=int(c[best_it]) if best_it >= 0 else int(best_in),
                no_more=int((not converged) and done + it_stop >= max_its))


def solve(prob, sets, best_inliers_in=0):
    """The constructor and one call of iterate with every member and argument it leaves behind, and the details of every set of the call."""
    S = Solver(prob)
    S.best_inliers = int(best_inliers_in)
    sets = np.asarray(sets, np.int32).reshape(-1, 3)
    I, N = len(sets), S.N
    if N < S.min_inliers:
        return dict(converged=0, it_stop=0, best_it=-1, best_inliers=S.best_inliers, improved=0, no_more=1, T12=np.zeros((4, 4), F),
                    R12=np.zeros((3, 3), F), t12=np.zeros(3, F), s12=F(0), best_mask=np.zeros(N, np.uint8), vbInliers=np.zeros(S.n1, np.uint8),
                    details=None, solver=S)
    hyps = [hypothesis(S, [int(v) for v in sets[k]]) for k in range(I)]
    checks = [check_inliers(S, h["T12"], h["T21"]) for h in hyps]
    out = iterate(S, I, sets, lambda k: (checks[k][0], k))
    b = out["best_it"]
    r = dict(out, best_inliers=S.best_inliers, solver=S)
    r["T12"] = np.array(hyps[b]["T12"], F) if b >= 0 else np.zeros((4, 4), F)
    r["R12"] = np.array(hyps[b]["R"], F) if b >= 0 else np.zeros((3, 3), F)
    r["t12"] = np.array(hyps[b]["t"], F) if b >= 0 else np.zeros(3, F)
    r["s12"] = F(hyps[b]["s"]) if b >= 0 else F(0)
    r["best_mask"] = np.array(checks[b][1], np.uint8) if b >= 0 else np.zeros(N, np.uint8)
    vb = np.zeros(S.n1, np.uint8)
    if out["converged"]:
        for i in range(N):
            if checks[b][1][i]:
                vb[S.idx1[i]] = 1                            # :231-233
    r["vbInliers"] = vb
    r["details"] = dict(counts=np.array([c[0] for c in checks], np.int32), T12=np.array([h["T12"] for h in hyps], F),
                        T21=np.array([h["T21"] for h in hyps], F), quat=np.array([h["q"] for h in hyps], F),
                        masks=np.array([c[1] for c in checks], np.uint8).reshape(I, N))
    return r
