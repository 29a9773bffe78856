"""A literal model of TwoViewReconstruction::Reconstruct (TwoViewReconstruction.cc:39-127) and of every member it calls, written after
the reference's text with real loops for the sequential sums, and of cv::SVD::compute (OpenCV's one-sided Jacobi for float) for any small
shape.  It shares no code with the product.

Numbers: a C `double` is a Python float.  A C `float` is a Python float that holds a float32 value, and every float operation is the
double operation rounded once more by f32(): for +, -, *, / and sqrt of float32 operands that second rounding changes nothing (a double
has more than 2*24 + 2 significand bits), so f32(a * b) IS the IEEE single product.  Rows that the reference updates element by element
are numpy float32 arrays, whose element-wise operations are the same IEEE single operations.

The cv::Mat expressions are folded as DESIGN.md section 2 says: mul_small (no transposed operand: the sum in float), mul_tA / mul_Bt (a
transposition flag: the sum in double), inv33, det33, `M / s`, `tp *= d`."""
import ctypes
import ctypes.util
import math

import numpy as np

FLT_MIN = float(np.finfo(np.float32).tiny)
FLT_EPSILON = float(np.finfo(np.float32).eps)
CV_PI = 3.1415926535897932384626433832795
F = np.float32
NAN, INF = float("nan"), float("inf")

NOT_INLIER, GOOD, LOW_PARALLAX, NONFINITE, BEHIND1, BEHIND2, REPROJ1, REPROJ2 = range(8)

_libm = ctypes.CDLL(ctypes.util.find_library("m"))
_libm.acosf.restype = ctypes.c_float
_libm.acosf.argtypes = [ctypes.c_float]


def acosf(x):
    return float(_libm.acosf(x))


def f32(x):
    with np.errstate(all="ignore"):
        return float(F(x))


def ddiv(a, b):
    """a / b as IEEE double division (Python raises on a zero divisor)"""
    if b == 0.0:
        if a != a or a == 0.0:
            return NAN
        return math.copysign(INF, a) * math.copysign(1.0, b)
    return a / b


def dsqrt(a):
    if a != a or a < 0.0:
        return NAN
    return math.sqrt(a)


def fadd(a, b): return f32(a + b)
def fsub(a, b): return f32(a - b)
def fmul(a, b): return f32(a * b)
def fdiv(a, b): return f32(ddiv(a, b))
def fsqrt(a): return f32(dsqrt(a))


def dot_double(x, y):
    """sum of products in double, ascending index; x, y float32 arrays or lists of float32 values"""
    s = 0.0
    for a, b in zip(np.asarray(x, dtype=np.float64).tolist(), np.asarray(y, dtype=np.float64).tolist()):
        s += a * b
    return s


# ---- cv::SVD::compute -----------------------------------------------------------------------------------------------------------------
def hypot(a, b):
    a, b = abs(a), abs(b)
    if a > b:
        b /= a
        return a * math.sqrt(1 + b * b)
    if b > 0:
        a /= b
        return b * math.sqrt(1 + a * a)
    return 0.0


def jacobi(At, m, n, n1):
    """JacobiSVDImpl_<float>: At a list of n1 float32 rows of length m (the first n hold the matrix's columns), returns (w, Vt); At is
    left holding the left vectors."""
    minval, eps = FLT_MIN, FLT_EPSILON * 2
    W = [dot_double(At[i], At[i]) for i in range(n)]
    Vt = [np.zeros(n, F) for _ in range(n)]
    for i in range(n):
        Vt[i][i] = 1
    for _ in range(max(m, 30)):
        changed = False
        for i in range(n - 1):
            for j in range(i + 1, n):
                a, b = W[i], W[j]
                p = dot_double(At[i], At[j])
                if abs(p) <= eps * dsqrt(a * b):
                    continue
                p *= 2
                beta = a - b
                gamma = hypot(p, beta)
                if beta < 0:
                    delta = (gamma - beta) * 0.5
                    s = f32(dsqrt(ddiv(delta, gamma)))
                    c = f32(ddiv(p, gamma * s * 2))
                else:
                    c = f32(dsqrt(ddiv(gamma + beta, gamma * 2)))
                    s = f32(ddiv(p, gamma * c * 2))
                c32, s32 = F(c), F(s)
                with np.errstate(all="ignore"):
                    t0 = c32 * At[i] + s32 * At[j]
                    t1 = -s32 * At[i] + c32 * At[j]
                    At[i], At[j] = t0, t1
                    W[i], W[j] = dot_double(t0, t0), dot_double(t1, t1)
                    changed = True
                    v0 = c32 * Vt[i] + s32 * Vt[j]
                    v1 = -s32 * Vt[i] + c32 * Vt[j]
                    Vt[i], Vt[j] = v0, v1
        if not changed:
            break
    W = [dsqrt(dot_double(At[i], At[i])) for i in range(n)]
    for i in range(n - 1):
        j = i
        for k in range(i + 1, n):
            if W[j] < W[k]:
                j = k
        if i != j:
            W[i], W[j] = W[j], W[i]
            At[i], At[j] = At[j], At[i]
            Vt[i], Vt[j] = Vt[j], Vt[i]
    w = [f32(x) for x in W]
    rng = 0x12345678
    for i in range(n1):
        sd = W[i] if i < n else 0.0
        ii = 0
        while ii < 100 and sd <= minval:
            val0 = f32(1.0 / m)
            row = []
            for _k in range(m):
                rng = ((rng & 0xFFFFFFFF) * 4164903690 + (rng >> 32)) & 0xFFFFFFFFFFFFFFFF
                row.append(val0 if (rng & 256) else -val0)
            for _it in range(2):
                for j in range(i):
                    Aj = At[j].astype(np.float64).tolist()
                    sd = 0.0
                    for k in range(m):
                        sd += fmul(row[k], Aj[k])          # a float product added to the double
                    asum = 0.0
                    for k in range(m):
                        t = f32(row[k] - sd * Aj[k])
                        row[k] = t
                        asum = fadd(asum, abs(t))
                    asum = fdiv(1.0, asum) if asum > eps * 100 else 0.0
                    row = [fmul(x, asum) for x in row]
            sd = 0.0
            for x in row:
                sd += x * x
            sd = math.sqrt(sd)
            At[i] = np.array(row, F)
            ii += 1
        s = f32(1 / sd if sd > minval else 0.0)
        with np.errstate(all="ignore"):
            At[i] = At[i] * F(s)
    return w, Vt


def svd(A):
    """cv::SVD::compute(A, w, u, vt, MODIFY_A | FULL_UV) of an m x n float32 matrix: (w [min(m,n)], u [m,m], vt [n,n])"""
    A = np.asarray(A, F)
    m, n = A.shape
    at = m < n
    if at:
        m, n = n, m
    rows = [np.zeros(m, F) for _ in range(m)]
    for i in range(n):
        rows[i] = (A[i, :] if at else A[:, i]).astype(F).copy()
    w, Vt = jacobi(rows, m, n, m)
    Am, Vm = np.array(rows, F).reshape(m, m), np.array(Vt, F).reshape(n, n)
    if not at:
        return np.array(w, F), Am.T.copy(), Vm
    return np.array(w, F), Vm.T.copy(), Am


# ---- the cv::Mat forms, on lists of rows of float32 values --------------------------------------------------------------------------------
def M(a):
    return [[float(v) for v in row] for row in np.asarray(a, F).reshape(3, -1)]


def mul_small(A, B, alpha=1.0):
    """alpha*A*B, no transposed operand, inner length 3: the sum of products in float, then (float)((double)sum*alpha + 0.0)"""
    out = []
    for i in range(len(A)):
        row = []
        for j in range(len(B[0])):
            s = fmul(A[i][0], B[0][j])
            for k in range(1, len(B)):
                s = fadd(s, fmul(A[i][k], B[k][j]))
            row.append(f32(s * alpha + 0.0))
        out.append(row)
    return out


def mul_tA(A, B, alpha=1.0):
    """alpha*A.t()*B: the generic path, the sum in double, rounded once"""
    out = []
    for i in range(3):
        row = []
        for j in range(len(B[0])):
            acc = 0.0
            for k in range(3):
                acc += A[k][i] * B[k][j]
            row.append(f32(alpha * acc))
        out.append(row)
    return out


def mul_Bt(A, B):
    out = []
    for i in range(3):
        row = []
        for j in range(3):
            acc = 0.0
            for k in range(3):
                acc += A[i][k] * B[j][k]
            row.append(f32(acc))
        out.append(row)
    return out


def det33(A):
    (a, b, c), (d, e, f), (g, h, i) = A
    return a * (e * i - f * h) - b * (d * i - f * g) + c * (d * h - e * g)


def inv33(A):
    cof = [[0.0] * 3 for _ in range(3)]
    for y in range(3):
        for x in range(3):
            r0, r1, c0, c1 = (x + 1) % 3, (x + 2) % 3, (y + 1) % 3, (y + 2) % 3
            cof[y][x] = A[r0][c0] * A[r1][c1] - A[r0][c1] * A[r1][c0]
    d = (A[0][0] * (A[1][1] * A[2][2] - A[1][2] * A[2][1]) - A[0][1] * (A[1][0] * A[2][2] - A[1][2] * A[2][0])
         + A[0][2] * (A[1][0] * A[2][1] - A[1][1] * A[2][0]))
    if d == 0.0:
        return [[0.0] * 3 for _ in range(3)]
    d = 1.0 / d
    return [[f32(cof[y][x] * d) for x in range(3)] for y in range(3)]


def transpose(A):
    return [[A[j][i] for j in range(len(A))] for i in range(len(A[0]))]


def neg(A):
    return [[-v for v in row] for row in A]


def sumsq(v):
    """the squares of a few float32 values accumulated in double, ascending (cv::norm)"""
    s = 0.0
    for x in v:
        s += x * x
    return s


def unit(v):
    """v / cv::norm(v)"""
    inv = ddiv(1.0, dsqrt(sumsq(v)))
    return [f32(x * inv) for x in v]


def svd33(A):
    w, u, vt = svd(np.array(A, F))
    return [float(x) for x in w], M(u), M(vt)


# ---- the members ---------------------------------------------------------------------------------------------------------------------------
def normalize(keys):
    """Normalize (:753-799): (normalised points [n][2] as lists, T)"""
    xs, ys = [float(v) for v in keys["x"]], [float(v) for v in keys["y"]]
    n = len(xs)
    meanX = meanY = 0.0
    for i in range(n):
        meanX = fadd(meanX, xs[i])
        meanY = fadd(meanY, ys[i])
    meanX, meanY = fdiv(meanX, float(n)), fdiv(meanY, float(n))
    px, py = [0.0] * n, [0.0] * n
    devX = devY = 0.0
    for i in range(n):
        px[i], py[i] = fsub(xs[i], meanX), fsub(ys[i], meanY)
        devX, devY = fadd(devX, abs(px[i])), fadd(devY, abs(py[i]))
    devX, devY = fdiv(devX, float(n)), fdiv(devY, float(n))
    sX, sY = f32(ddiv(1.0, devX)), f32(ddiv(1.0, devY))
    pts = [(fmul(px[i], sX), fmul(py[i], sY)) for i in range(n)]
    T = [[sX, 0.0, fmul(-meanX, sX)], [0.0, sY, fmul(-meanY, sY)], [0.0, 0.0, 1.0]]
    return pts, T


def compute_H21(P1, P2):
    A = np.zeros((16, 9), F)
    for i in range(8):
        (u1, v1), (u2, v2) = P1[i], P2[i]
        A[2 * i] = [0, 0, 0, -u1, -v1, -1, fmul(v2, u1), fmul(v2, v1), v2]
        A[2 * i + 1] = [u1, v1, 1, 0, 0, 0, fmul(-u2, u1), fmul(-u2, v1), -u2]
    _, _, vt = svd(A)
    return M(vt[8].reshape(3, 3))


def compute_F21(P1, P2):
    A = np.zeros((8, 9), F)
    for i in range(8):
        (u1, v1), (u2, v2) = P1[i], P2[i]
        A[i] = [fmul(u2, u1), fmul(u2, v1), u2, fmul(v2, u1), fmul(v2, v1), v2, u1, v1, 1]
    _, _, vt = svd(A)
    w, u, vt = svd33(M(vt[8].reshape(3, 3)))
    w[2] = 0.0
    D = [[w[0], 0.0, 0.0], [0.0, w[1], 0.0], [0.0, 0.0, w[2]]]
    return mul_small(mul_small(u, D), vt)


def _f32div_double(den):
    """(float)(1.0 / den) for a float32 array den"""
    with np.errstate(all="ignore"):
        return (1.0 / den.astype(np.float64)).astype(F)


def _score(terms, adds):
    """score += term, in the reference's order: match ascending, first image then second"""
    score = 0.0
    t, a = [x.astype(np.float64).tolist() for x in terms], [x.tolist() for x in adds]
    for i in range(len(t[0])):
        if a[0][i]:
            score = fadd(score, t[0][i])
        if a[1][i]:
            score = fadd(score, t[1][i])
    return score


def check_homography(H21, H12, mx, sigma):
    """CheckHomography (:310-393): (score, inliers); mx = (u1, v1, u2, v2) float32 arrays"""
    u1, v1, u2, v2 = mx
    h, hi = [[F(v) for v in r] for r in H21], [[F(v) for v in r] for r in H12]
    th = F(5.991)
    invSigmaSquare = F(ddiv(1.0, fmul(sigma, sigma)))
    with np.errstate(all="ignore"):
        w2in1inv = _f32div_double(hi[2][0] * u2 + hi[2][1] * v2 + hi[2][2])
        u2in1 = (hi[0][0] * u2 + hi[0][1] * v2 + hi[0][2]) * w2in1inv
        v2in1 = (hi[1][0] * u2 + hi[1][1] * v2 + hi[1][2]) * w2in1inv
        chi1 = ((u1 - u2in1) * (u1 - u2in1) + (v1 - v2in1) * (v1 - v2in1)) * invSigmaSquare
        w1in2inv = _f32div_double(h[2][0] * u1 + h[2][1] * v1 + h[2][2])
        u1in2 = (h[0][0] * u1 + h[0][1] * v1 + h[0][2]) * w1in2inv
        v1in2 = (h[1][0] * u1 + h[1][1] * v1 + h[1][2]) * w1in2inv
        chi2 = ((u2 - u1in2) * (u2 - u1in2) + (v2 - v1in2) * (v2 - v1in2)) * invSigmaSquare
        add1, add2 = ~(chi1 > th), ~(chi2 > th)
        score = _score((th - chi1, th - chi2), (add1, add2))
    return score, add1 & add2


def check_fundamental(F21, mx, sigma):
    """CheckFundamental (:395-473)"""
    u1, v1, u2, v2 = mx
    f = [[F(v) for v in r] for r in F21]
    th, thScore = F(3.841), F(5.991)
    invSigmaSquare = F(ddiv(1.0, fmul(sigma, sigma)))
    with np.errstate(all="ignore"):
        a2 = f[0][0] * u1 + f[0][1] * v1 + f[0][2]
        b2 = f[1][0] * u1 + f[1][1] * v1 + f[1][2]
        c2 = f[2][0] * u1 + f[2][1] * v1 + f[2][2]
        num2 = a2 * u2 + b2 * v2 + c2
        chi1 = (num2 * num2 / (a2 * a2 + b2 * b2)) * invSigmaSquare
        a1 = f[0][0] * u2 + f[1][0] * v2 + f[2][0]
        b1 = f[0][1] * u2 + f[1][1] * v2 + f[2][1]
        c1 = f[0][2] * u2 + f[1][2] * v2 + f[2][2]
        num1 = a1 * u1 + b1 * v1 + c1
        chi2 = (num1 * num1 / (a1 * a1 + b1 * b1)) * invSigmaSquare
        add1, add2 = ~(chi1 > th), ~(chi2 > th)
        score = _score((thScore - chi1, thScore - chi2), (add1, add2))
    return score, add1 & add2


class Problem:
    """mvKeys1 / mvKeys2 / mvMatches12 as Reconstruct fills them (:42-62)"""

    def __init__(self, keys1, keys2, matches12):
        self.keys1, self.keys2 = keys1, keys2
        self.matches = [(i, int(j)) for i, j in enumerate(matches12) if j >= 0]
        self.N = len(self.matches)
        a, b = [p[0] for p in self.matches], [p[1] for p in self.matches]
        self.mx = (keys1["x"][a].astype(F), keys1["y"][a].astype(F), keys2["x"][b].astype(F), keys2["y"][b].astype(F))


def find_models(Q, sigma, iterations, sets):
    """FindHomography and FindFundamental (:129-228): every iteration's matrices and scores, and the running best of each loop"""
    vPn1, T1 = normalize(Q.keys1)
    vPn2, T2 = normalize(Q.keys2)
    T2inv, T2t = inv33(T2), transpose(T2)
    I = iterations
    out = dict(H21=np.zeros((I, 3, 3), F), H12=np.zeros((I, 3, 3), F), F21=np.zeros((I, 3, 3), F), score=np.zeros((2, I), F),
               best_it=[-1, -1], masks=np.zeros((2, Q.N), bool), S=[0.0, 0.0], best=[None, None])
    for model in range(2):
        score = 0.0
        for it in range(I):
            P1 = [vPn1[Q.matches[idx][0]] for idx in sets[it]]
            P2 = [vPn2[Q.matches[idx][1]] for idx in sets[it]]
            if model == 0:
                H21i = mul_small(mul_small(T2inv, compute_H21(P1, P2)), T1)
                H12i = inv33(H21i)
                cur, inl = check_homography(H21i, H12i, Q.mx, sigma)
                out["H21"][it], out["H12"][it], Mi = np.array(H21i, F), np.array(H12i, F), H21i
            else:
                F21i = mul_small(mul_small(T2t, compute_F21(P1, P2)), T1)
                cur, inl = check_fundamental(F21i, Q.mx, sigma)
                out["F21"][it], Mi = np.array(F21i, F), F21i
            out["score"][model, it] = cur
            if cur > score:
                score, out["best_it"][model], out["masks"][model], out["best"][model] = cur, it, inl, Mi
        out["S"][model] = score
    return out


def triangulate(P1, P2, u1, v1, u2, v2):
    """Triangulate (:738-751): x3D or None when a coordinate is not finite is the caller's test"""
    A = np.zeros((4, 4), F)
    with np.errstate(all="ignore"):
        A[0] = F(u1) * P1[2] - P1[0]
        A[1] = F(v1) * P1[2] - P1[1]
        A[2] = F(u2) * P2[2] - P2[0]
        A[3] = F(v2) * P2[2] - P2[1]
    _, _, vt = svd(A)
    v = [float(x) for x in vt[3]]
    inv = ddiv(1.0, v[3])
    return [f32(v[k] * inv) for k in range(3)]


def check_rt(Q, inliers, K, sigma, R, t):
    """CheckRT (:802-911) for one hypothesis: dict(vP3D [n1,3], vbGood [n1], status [N], nGood, cos_rank, parallax)"""
    K, R, t = M(K), M(R), [float(v) for v in np.asarray(t, F).reshape(3)]
    fx, fy, cx, cy = K[0][0], K[1][1], K[0][2], K[1][2]
    th2 = f32(4.0 * fmul(sigma, sigma))
    n1 = len(Q.keys1)
    vP3D, vbGood, status, cosv = np.zeros((n1, 3), F), np.zeros(n1, bool), np.zeros(Q.N, np.uint8), []
    z1, z2, cosines = np.full(Q.N, np.nan), np.full(Q.N, np.nan), np.full(Q.N, np.nan)   # for the tests' scene properties only
    P1 = np.array([row + [0.0] for row in K], F)
    Rt = [R[i] + [t[i]] for i in range(3)]
    P2 = np.array(mul_small(K, Rt), F)
    O2 = [row[0] for row in mul_tA(R, [[v] for v in t], -1.0)]
    u1s, v1s, u2s, v2s = [a.astype(np.float64).tolist() for a in Q.mx]
    for i in range(Q.N):
        if not inliers[i]:
            status[i] = NOT_INLIER
            continue
        u1, v1, u2, v2 = u1s[i], v1s[i], u2s[i], v2s[i]
        p = triangulate(P1, P2, u1, v1, u2, v2)
        if not all(math.isfinite(c) for c in p):
            status[i] = NONFINITE
            continue
        normal1 = [fsub(c, 0.0) for c in p]
        dist1 = f32(dsqrt(sumsq(normal1)))
        normal2 = [fsub(p[k], O2[k]) for k in range(3)]
        dist2 = f32(dsqrt(sumsq(normal2)))
        dot = 0.0
        for k in range(3):
            dot += normal1[k] * normal2[k]
        cosParallax = f32(ddiv(dot, fmul(dist1, dist2)))
        z1[i], cosines[i] = p[2], cosParallax
        if p[2] <= 0 and cosParallax < 0.99998:
            status[i] = BEHIND1
            continue
        p2 = []
        for r in range(3):
            s = fadd(fadd(fmul(R[r][0], p[0]), fmul(R[r][1], p[1])), fmul(R[r][2], p[2]))
            p2.append(f32(s * 1.0 + t[r] * 1.0))
        z2[i] = p2[2]
        if p2[2] <= 0 and cosParallax < 0.99998:
            status[i] = BEHIND2
            continue
        invZ1 = f32(ddiv(1.0, p[2]))
        im1x, im1y = fadd(fmul(fmul(fx, p[0]), invZ1), cx), fadd(fmul(fmul(fy, p[1]), invZ1), cy)
        e1 = fadd(fmul(fsub(im1x, u1), fsub(im1x, u1)), fmul(fsub(im1y, v1), fsub(im1y, v1)))
        if e1 > th2:
            status[i] = REPROJ1
            continue
        invZ2 = f32(ddiv(1.0, p2[2]))
        im2x, im2y = fadd(fmul(fmul(fx, p2[0]), invZ2), cx), fadd(fmul(fmul(fy, p2[1]), invZ2), cy)
        e2 = fadd(fmul(fsub(im2x, u2), fsub(im2x, u2)), fmul(fsub(im2y, v2), fsub(im2y, v2)))
        if e2 > th2:
            status[i] = REPROJ2
            continue
        cosv.append(cosParallax)
        vP3D[Q.matches[i][0]] = p
        if cosParallax < 0.99998:
            vbGood[Q.matches[i][0]] = True
            status[i] = GOOD
        else:
            status[i] = LOW_PARALLAX
    nGood, cos_rank, parallax = len(cosv), 0.0, 0.0
    if nGood > 0:
        cosv.sort()
        cos_rank = cosv[min(50, nGood - 1)]
        parallax = f32(fmul(acosf(cos_rank), 180.0) / CV_PI)
    return dict(vP3D=vP3D, vbGood=vbGood, status=status, nGood=nGood, cos_rank=cos_rank, parallax=parallax, z1=z1, z2=z2, cos=cosines,
                sorted_cos=cosv)


def decompose_E(E):
    w, u, vt = svd33(E)
    t = unit([u[i][2] for i in range(3)])
    W = [[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]]
    R1 = mul_small(mul_small(u, W), vt)
    if det33(R1) < 0:
        R1 = neg(R1)
    R2 = mul_small(mul_Bt(u, W), vt)
    if det33(R2) < 0:
        R2 = neg(R2)
    return R1, R2, t


def hypotheses_F(F21, K):
    E21 = mul_small(mul_tA(K, F21), K)
    R1, R2, t = decompose_E(E21)
    t2 = [-v for v in t]
    return [R1, R2, R1, R2], [t, t, t2, t2]


def hypotheses_H(H21, K):
    """the eight (R, t) of ReconstructH (:588-690), or None at :601"""
    A = mul_small(mul_small(inv33(K), H21), K)
    w, U, Vt = svd33(A)
    s = f32(det33(U) * det33(Vt))
    d1, d2, d3 = w
    if fdiv(d1, d2) < 1.00001 or fdiv(d2, d3) < 1.00001:
        return None
    sq = lambda a: fmul(a, a)
    aux1 = fsqrt(fdiv(fsub(sq(d1), sq(d2)), fsub(sq(d1), sq(d3))))
    aux3 = fsqrt(fdiv(fsub(sq(d2), sq(d3)), fsub(sq(d1), sq(d3))))
    x1, x3 = [aux1, aux1, -aux1, -aux1], [aux3, -aux3, aux3, -aux3]
    root = fsqrt(fmul(fsub(sq(d1), sq(d2)), fsub(sq(d2), sq(d3))))
    aux_stheta = fdiv(root, fmul(fadd(d1, d3), d2))
    ctheta = fdiv(fadd(sq(d2), fmul(d1, d3)), fmul(fadd(d1, d3), d2))
    stheta = [aux_stheta, -aux_stheta, -aux_stheta, aux_stheta]
    aux_sphi = fdiv(root, fmul(fsub(d1, d3), d2))
    cphi = fdiv(fsub(fmul(d1, d3), sq(d2)), fmul(fsub(d1, d3), d2))
    sphi = [aux_sphi, -aux_sphi, -aux_sphi, aux_sphi]
    vR, vt = [], []
    for h in range(8):
        i = h & 3
        if h < 4:
            Rp = [[ctheta, 0.0, -stheta[i]], [0.0, 1.0, 0.0], [stheta[i], 0.0, ctheta]]
            tp, d = [x1[i], 0.0, -x3[i]], fsub(d1, d3)
        else:
            Rp = [[cphi, 0.0, sphi[i]], [0.0, -1.0, 0.0], [sphi[i], 0.0, -cphi]]
            tp, d = [x1[i], 0.0, x3[i]], fadd(d1, d3)
        vR.append(mul_small(mul_small(U, Rp, s), Vt))
        tp = [f32(v * d) for v in tp]
        t = [row[0] for row in mul_small(U, [[v] for v in tp])]
        vt.append(unit(t))
    return vR, vt


def select_F(nGood, parallax, N):
    maxGood = max(nGood)
    nMinGood = max(int(0.9 * N), 50)
    nsimilar = sum(1 for g in nGood if g > 0.7 * maxGood)
    if maxGood < nMinGood or nsimilar > 1:
        return -1
    for i in range(4):
        if maxGood == nGood[i]:
            return i if parallax[i] > 1.0 else -1
    return -1


def select_H(nGood, parallax, N):
    bestGood, secondBestGood, best, bestParallax = 0, 0, -1, -1.0
    for i in range(8):
        if nGood[i] > bestGood:
            secondBestGood, bestGood, best, bestParallax = bestGood, nGood[i], i, parallax[i]
        elif nGood[i] > secondBestGood:
            secondBestGood = nGood[i]
    if secondBestGood < 0.75 * bestGood and bestParallax >= 1.0 and bestGood > 50 and bestGood > 0.9 * N:
        return best
    return -1


def reconstruct(keys1, keys2, matches12, K, sigma, iterations, sets):
    """Reconstruct (:39-127): dict(ok, R21, t21, vP3D, vbTriangulated) plus everything the product's `details` holds, and `why`"""
    Q = Problem(keys1, keys2, matches12)
    K = M(K)
    models = find_models(Q, sigma, iterations, sets)
    SH, SF = models["S"]
    zero = [[0.0] * 3] * 3
    out = dict(ok=False, SH=SH, SF=SF, best_it=models["best_it"], score=models["score"], inliersH=models["masks"][0],
               inliersF=models["masks"][1], H21=np.array(models["best"][0] or zero, F), F21=np.array(models["best"][1] or zero, F),
               used_H=-1, nhyp=0, chosen=-1, R=np.zeros((8, 3, 3), F), t=np.zeros((8, 3), F), nGood=np.zeros(8, np.int32),
               parallax=np.zeros(8, F), status=np.zeros((8, Q.N), np.uint8), why="SH+SF == 0", models=models)
    if fadd(SH, SF) == 0.0:
        return out
    RH = fdiv(SH, fadd(SH, SF))
    model = 0 if RH > 0.50 else 1
    out["used_H"] = int(model == 0)
    inl = models["masks"][model]
    N = int(inl.sum())
    hyp = hypotheses_H(models["best"][0], K) if model == 0 else hypotheses_F(models["best"][1], K)
    if hyp is None:
        out["why"] = "d1/d2 or d2/d3 < 1.00001"
        return out
    vR, vt = hyp
    out["nhyp"] = len(vR)
    checks = [check_rt(Q, inl, K, sigma, vR[h], vt[h]) for h in range(len(vR))]
    for h, c in enumerate(checks):
        out["R"][h], out["t"][h], out["nGood"][h], out["parallax"][h], out["status"][h] = np.array(vR[h], F), vt[h], c["nGood"], c["parallax"], c["status"]
    nGood, parallax = [c["nGood"] for c in checks], [c["parallax"] for c in checks]
    chosen = select_H(nGood, parallax, N) if model == 0 else select_F(nGood, parallax, N)
    out["chosen"], out["checks"], out["N_inliers"] = chosen, checks, N
    if chosen < 0:
        maxGood = max(nGood)
        if model == 1:
            nsimilar = sum(1 for g in nGood if g > 0.7 * maxGood)
            out["why"] = ("nsimilar > 1" if nsimilar > 1 and maxGood >= max(int(0.9 * N), 50) else
                          "maxGood < nMinGood" if maxGood < max(int(0.9 * N), 50) else "parallax")
        else:
            second = sorted(nGood)[-2]
            out["why"] = ("parallax" if second < 0.75 * maxGood and maxGood > 50 and maxGood > 0.9 * N else "counts")
        return out
    out.update(ok=True, why="", R21=np.array(vR[chosen], F), t21=np.array(vt[chosen], F), vP3D=checks[chosen]["vP3D"],
               vbTriangulated=checks[chosen]["vbGood"])
    return out


def draw_sets(N, iterations, rand):
    """The set-drawing loop of Reconstruct (:77-96) over a caller's RandomInt(min, max)"""
    sets = np.zeros((iterations, 8), np.int32)
    for it in range(iterations):
        avail = list(range(N))
        for j in range(8):
            randi = rand(0, len(avail) - 1)
            sets[it, j] = avail[randi]
            avail[randi] = avail[-1]
            avail.pop()
    return sets
