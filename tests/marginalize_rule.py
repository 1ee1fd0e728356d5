"""The rule marginalizing node removal is pinned to (the reference removes a vertex with its edges and transfers nothing, so there is
no reference figure): when node v leaves, its constraints are composed through it into constraints among its neighbours.

The rule reads and writes only constraints (a, b, z, Omega): z is pose b in the frame of a (oracle/spa.py), Omega the information,
Sigma = Omega^-1.  No poses, no linearisation point.  With R(t) the 2 x 2 rotation and R'(t) its derivative:

  inverse of (z = (t, th), Sigma):  z' = (-R(th)^T t, -th),  Sigma' = J Sigma J^T,  J = [[-R^T, -R'(th)^T t], [0, -1]]
  compose z1 (+) z2:                t = t1 + R(th1) t2,  th = normalize(th1 + th2),
                                    Sigma = w J1 Sigma1 J1^T + J2 Sigma2 J2^T,  J1 = [[I, R'(th1) t2], [0, 1]],  J2 = [[R(th1), 0], [0, 1]]
  fuse (same ordered pair; one stored the other way round is inverted first):
                                    Omega = Omega1 + Omega2,  z = z1 + Omega^-1 Omega2 (z2 - z1), the angle difference normalized

marginalize(cons, v):
  1. parallel constraints between v and one neighbour are fused in constraint order onto the first: one entry per neighbour, in
     the order of v's first constraint to each;
  2. the hub h is the entry whose information (as stored or as fused, before orienting) has the largest determinant, ties to the
     lowest node id;
  3. every entry is oriented v -> n_i (inverted where it is stored n_i -> v);
  4. for every i != h the new constraint h -> n_i is inverse(v -> h) (+) (v -> n_i), the hub's term weighted w = d - 1: the d - 1
     new constraints, taken as independent, then carry no more information than the exact dense marginal, because
     ((d-1) I - 1 1^T) (x) Sigma_h is positive semidefinite; for d = 2 this is the exact first-order marginal;
  5. where h and n_i already share a constraint (either direction) the new one is fused into the first such constraint, which
     keeps its direction and its place; otherwise it is appended, in neighbour order;
  6. v's constraints leave.
A node with d <= 1 is simply removed.  A list of nodes is processed in list order.

Every operation is written out element by element in one fixed order and works in the dtype of its input, so that the same text
gives the float64 rule and its np.longdouble restatement: ref_err (the convention of tests/covariance_rule.py) is the largest
relative Frobenius difference between the two over the emitted z and Omega."""
import numpy as np

LD = np.longdouble
EPS = 2.0 ** -52


def _pi(T):
    return T(4) * np.arctan(T(1))


def normalize(th):
    """ceres_utils.h:27-32, as oracle.spa.normalize_angle: [-pi, pi)"""
    T = type(th)
    pi = _pi(T)
    return th - T(2) * pi * np.floor((th + pi) / (T(2) * pi))


def mm(A, B):
    return A[:, 0:1] * B[0:1, :] + A[:, 1:2] * B[1:2, :] + A[:, 2:3] * B[2:3, :]


def mirror(M):
    """the symmetric matrix that has M's upper triangle (what the solver stores)"""
    out = M.copy()
    out[1, 0] = M[0, 1]; out[2, 0] = M[0, 2]; out[2, 1] = M[1, 2]
    return out


def congruence(J, S):
    return mirror(mm(mm(J, S), J.T.copy()))


def det3(m):
    return m[0, 0] * (m[1, 1] * m[2, 2] - m[1, 2] * m[1, 2]) - m[0, 1] * (m[0, 1] * m[2, 2] - m[1, 2] * m[0, 2]) + \
        m[0, 2] * (m[0, 1] * m[1, 2] - m[1, 1] * m[0, 2])


def inv3(m):
    """inverse of a symmetric 3 x 3 by cofactors of its upper triangle"""
    T = m.dtype.type
    c00 = m[1, 1] * m[2, 2] - m[1, 2] * m[1, 2]
    c01 = m[0, 2] * m[1, 2] - m[0, 1] * m[2, 2]
    c02 = m[0, 1] * m[1, 2] - m[0, 2] * m[1, 1]
    c11 = m[0, 0] * m[2, 2] - m[0, 2] * m[0, 2]
    c12 = m[0, 1] * m[0, 2] - m[0, 0] * m[1, 2]
    c22 = m[0, 0] * m[1, 1] - m[0, 1] * m[0, 1]
    r = T(1) / (m[0, 0] * c00 + m[0, 1] * c01 + m[0, 2] * c02)
    return np.array([[c00 * r, c01 * r, c02 * r], [c01 * r, c11 * r, c12 * r], [c02 * r, c12 * r, c22 * r]], dtype=m.dtype)


def inverse(z, S):
    T = z.dtype.type
    c, s = np.cos(z[2]), np.sin(z[2])
    x, y = z[0], z[1]
    zi = np.array([-(c * x + s * y), -(c * y - s * x), -z[2]], dtype=z.dtype)
    J = np.array([[-c, -s, s * x - c * y], [s, -c, c * x + s * y], [T(0), T(0), T(-1)]], dtype=z.dtype)
    return zi, congruence(J, S)


def compose(z1, S1, z2, S2, w):
    T = z1.dtype.type
    c, s = np.cos(z1[2]), np.sin(z1[2])
    x, y = z2[0], z2[1]
    z = np.array([z1[0] + (c * x - s * y), z1[1] + (s * x + c * y), normalize(z1[2] + z2[2])], dtype=z1.dtype)
    J1 = np.array([[T(1), T(0), -(s * x) - c * y], [T(0), T(1), c * x - s * y], [T(0), T(0), T(1)]], dtype=z1.dtype)
    J2 = np.array([[c, -s, T(0)], [s, c, T(0)], [T(0), T(0), T(1)]], dtype=z1.dtype)
    return z, mirror(T(w) * congruence(J1, S1) + congruence(J2, S2))


def flip(z, O):
    """the same constraint stored the other way round"""
    zi, Si = inverse(z, inv3(O))
    return zi, inv3(Si)


def fuse(z1, O1, z2, O2):
    O = mirror(O1 + O2)
    d = z2 - z1
    d[2] = normalize(d[2])
    v = mm(O2, d.reshape(3, 1))
    return z1 + mm(inv3(O), v).reshape(3), O


def make(cons, dtype=np.float64):
    """[(a, b, z, Omega)] -> the rule's own list (copies, in `dtype`, Omega mirrored from its upper triangle)"""
    return [[int(a), int(b), np.asarray(z, dtype=dtype).copy(), mirror(np.asarray(O, dtype=dtype).reshape(3, 3))] for a, b, z, O in cons]


def entries_of(cons, v):
    """step 1 without the arithmetic: [(neighbour, [positions in cons])] in the order of v's first constraint to each"""
    order, where = [], {}
    for k, (a, b, _, _) in enumerate(cons):
        if a == v or b == v:
            n = b if a == v else a
            if n not in where:
                where[n] = len(order)
                order.append((n, []))
            order[where[n]][1].append(k)
    return order


def marginalize(cons, v):
    """in place; returns dict(d, hub, added=[positions], fused=[positions]) with positions in the list as it is afterwards"""
    ents = entries_of(cons, v)
    d = len(ents)
    info = dict(d=d, hub=None, added=[], fused=[])
    dead = {k for _, ks in ents for k in ks}
    if d >= 2:
        fusedv = []
        for n, ks in ents:
            a0, _, z, O = cons[ks[0]]
            z, O = z.copy(), O.copy()
            for k in ks[1:]:
                a, _, z2, O2 = cons[k]
                if a != a0:
                    z2, O2 = flip(z2, O2)
                z, O = fuse(z, O, z2, O2)
            fusedv.append((n, a0 == v, z, O))
        dets = [det3(O) for _, _, _, O in fusedv]
        h = 0
        for i in range(1, d):
            if dets[i] > dets[h] or (dets[i] == dets[h] and fusedv[i][0] < fusedv[h][0]):
                h = i
        oriented = []
        for n, forward, z, O in fusedv:
            S = inv3(O)
            oriented.append((z, S) if forward else inverse(z, S))
        zh, Sh = inverse(*oriented[h])
        hub = fusedv[h][0]
        info["hub"] = hub
        fused_at, appended = [], []
        for i in range(d):
            if i == h:
                continue
            n = fusedv[i][0]
            z, S = compose(zh, Sh, oriented[i][0], oriented[i][1], d - 1)
            O = inv3(S)
            first = next((k for k, (a, b, _, _) in enumerate(cons) if k not in dead and ((a == hub and b == n) or (a == n and b == hub))), None)
            if first is None:
                appended.append([hub, n, z, O])
            else:
                if cons[first][0] != hub:
                    z, O = flip(z, O)
                cons[first][2], cons[first][3] = fuse(cons[first][2], cons[first][3], z, O)
                fused_at.append(first)
        cons.extend(appended)
        keep = [k for k in range(len(cons)) if k not in dead]
        new_pos = {k: p for p, k in enumerate(keep)}
        info["fused"] = [new_pos[k] for k in fused_at]
        info["added"] = [new_pos[k] for k in range(len(cons) - len(appended), len(cons))]
    cons[:] = [c for k, c in enumerate(cons) if k not in dead]
    return info


def marginalize_list(cons, nodes):
    return [marginalize(cons, int(v)) for v in nodes]


def rel_fro(got, want):
    want = np.asarray(want, dtype=LD)
    diff = np.asarray(got, dtype=LD) - want
    den = float(np.sqrt(np.sum(want * want)))
    num = float(np.sqrt(np.sum(diff * diff)))
    return num / den if den > 0.0 else (0.0 if num == 0.0 else np.inf)


def ref_err(cons64, consld):
    """largest relative Frobenius difference of a z or an Omega between the float64 rule's list and the long double one's"""
    assert [(c[0], c[1]) for c in cons64] == [(c[0], c[1]) for c in consld]
    worst = 0.0
    for c, r in zip(cons64, consld):
        worst = max(worst, rel_fro(c[2], r[2]), rel_fro(c[3], r[3]))
    return worst


def tolerance(err):
    """tests/covariance_rule.py's: a block of the library may be this far (relative Frobenius) from the float64 rule"""
    return max(8.0 * err, 64.0 * EPS)


def components(cons, nodes):
    """number of connected components that hold one of `nodes`, under the constraints"""
    parent = {int(n): int(n) for n in nodes}

    def find(x):
        parent.setdefault(x, x)
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    for a, b, _, _ in cons:
        parent[find(a)] = find(b)
    return len({find(int(n)) for n in nodes})
