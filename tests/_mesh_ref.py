"""The numpy definition of the depth mesh (include/falnet_hip.h: falnet_mesh_build), for tests/test_mesh_host.py, tests/test_gpu_mesh.py and
tools/bench_mesh.py.  Written from the definition's text, array-wise: every f32 step is one numpy f32 operation (numpy does not fuse a multiply with an
add), every f64 step of the normals one f64 operation in the stated order.

  build_ref(img, disp, focal, baseline, ...)   -> (vertex records (nv, 15 | 27) u8, face records (nf, 13) u8, info)
  family(name, H, W)                           the seeded input families the tests run: dict(img, disp, focal, baseline, kw)
  parse_ply(path)                              a small PLY reader: (vertex structured array, faces (nf, 3) int32, header dict)"""
import numpy as np

F32 = np.float32
MEAN = (0.411, 0.432, 0.45)
VERTEX = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("red", "u1"), ("green", "u1"), ("blue", "u1")])
VERTEX_N = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4"), ("red", "u1"), ("green", "u1"), ("blue", "u1")])
FACE = np.dtype([("n", "u1"), ("v", "<i4", (3,))])
assert VERTEX.itemsize == 15 and VERTEX_N.itemsize == 27 and FACE.itemsize == 13
FAMILIES = ("plane", "step", "holes", "random", "quant", "score", "inf-jump")


def vertices_f32(img, disp, focal, baseline, mean=MEAN, rgb_scale=255.0):
    """The point cloud's vertex chain per pixel: PLY x, y, z (= the cloud's x, capped z, -y) as f32 (H, W) maps and the three colour bytes (H, W, 3)."""
    H, W = disp.shape
    fb = F32(float(focal) * float(baseline))  # the product in double, rounded once
    f = F32(focal)
    with np.errstate(all="ignore"):
        z = fb / (disp.astype(F32) + F32(1e-4))
        u = (np.arange(W, dtype=F32) + F32(0.5)).reshape(1, W)
        v = (np.arange(H, dtype=F32) + F32(0.5)).reshape(H, 1)
        x = ((u - F32(W / 2.0)) / f) * z
        y = ((v - F32(H / 2.0)) / f) * z
        zc = np.where(z < 0, F32(0), z)
        zc = np.where(zc > 200, F32(200), zc)
        col = (img.astype(F32) + np.asarray(mean, F32).reshape(3, 1, 1)) * F32(rgb_scale)
        rgb = np.where(col >= 255, 255, np.where(col >= 1, np.trunc(col), 0)).astype(np.uint8)  # int(), saturated
    assert x.dtype == F32 and zc.dtype == F32 and y.dtype == F32
    return x, zc, -y, np.ascontiguousarray(rgb.transpose(1, 2, 0))


def build_ref(img, disp, focal, baseline, max_jump=0.05, min_depth=0.0, max_depth=80.0, score=None, threshold=None, normals=False, mean=MEAN,
              rgb_scale=255.0):
    """img (3, H, W) f32, disp (H, W) f32 -> (vertices (nv, 15 | 27) u8, faces (nf, 13) u8, info).  info: 'used' the pixel indices of the vertices,
    'faces' the (nf, 3) new indices, 'xyz' the (nv, 3) f32 positions."""
    if not (0.0 <= min_depth < max_depth < 200.0) or not max_jump >= 0.0:
        raise ValueError("need 0 <= min_depth < max_depth < 200 and max_jump >= 0")
    H, W = disp.shape
    n = H * W
    px, py, pz, rgb = vertices_f32(img, disp, focal, baseline, mean, rgb_scale)
    z = py  # the capped f32 depth
    with np.errstate(all="ignore"):
        valid = (z > F32(min_depth)) & (z <= F32(max_depth))
        if score is not None:
            valid &= score.astype(F32) >= F32(threshold)
    ratio = F32(1.0 + float(max_jump))
    if H < 2 or W < 2:
        faces_old = np.zeros((0, 3), np.int64)
        bc = kept = None
    else:
        g = np.arange(n, dtype=np.int64).reshape(H, W)
        ia, ib, ic, id_ = g[:-1, :-1], g[:-1, 1:], g[1:, :-1], g[1:, 1:]
        za, zb, zc, zd = z[:-1, :-1], z[:-1, 1:], z[1:, :-1], z[1:, 1:]
        va, vb, vc, vd = valid[:-1, :-1], valid[:-1, 1:], valid[1:, :-1], valid[1:, 1:]
        ninv = (~va).astype(int) + (~vb) + (~vc) + (~vd)
        with np.errstate(all="ignore"):
            all_valid_bc = ~(np.abs(za - zd) <= np.abs(zb - zc))  # a tie goes to a-d
            bc = np.where(ninv == 1, ~va | ~vd, all_valid_bc)

            def edge(p, q):
                return np.maximum(p, q) <= np.minimum(p, q) * ratio

            e_ac, e_cd, e_ad, e_db, e_ba, e_cb = edge(za, zc), edge(zc, zd), edge(za, zd), edge(zd, zb), edge(zb, za), edge(zc, zb)
        t0 = np.where(bc, va & vc & vb & e_ac & e_cb & e_ba, va & vc & vd & e_ac & e_cd & e_ad)
        t1 = np.where(bc, vb & vc & vd & e_cb & e_cd & e_db, va & vd & vb & e_ad & e_db & e_ba)
        t0 &= ninv < 2
        t1 &= ninv < 2
        tri0 = np.stack([ia, ic, np.where(bc, ib, id_)], -1)
        tri1 = np.stack([np.where(bc, ib, ia), np.where(bc, ic, id_), np.where(bc, id_, ib)], -1)
        tris = np.stack([tri0, tri1], 2).reshape(-1, 2, 3)  # quad order, T0 before T1
        kept = np.stack([t0, t1], -1)
        faces_old = tris[kept.reshape(-1, 2)]
    used = np.zeros(n, bool)
    used[faces_old.reshape(-1)] = True
    new_index = np.cumsum(used) - 1
    faces = new_index[faces_old].astype(np.int32).reshape(-1, 3)
    idx = np.flatnonzero(used)
    vert = np.zeros(len(idx), VERTEX_N if normals else VERTEX)
    vert["x"], vert["y"], vert["z"] = px.reshape(-1)[idx], py.reshape(-1)[idx], pz.reshape(-1)[idx]
    vert["red"], vert["green"], vert["blue"] = (rgb.reshape(-1, 3)[idx, k] for k in range(3))
    if normals:
        nrm = vertex_normals(px, py, pz, bc, kept) if kept is not None else np.zeros((H, W, 3), F32)
        vert["nx"], vert["ny"], vert["nz"] = (nrm.reshape(-1, 3)[idx, k] for k in range(3))
    rec = np.zeros(len(faces), FACE)
    rec["n"], rec["v"] = 3, faces
    info = dict(used=idx, faces=faces, xyz=np.stack([vert["x"], vert["y"], vert["z"]], -1) if len(idx) else np.zeros((0, 3), F32))
    return (np.frombuffer(vert.tobytes(), np.uint8).reshape(-1, vert.dtype.itemsize), np.frombuffer(rec.tobytes(), np.uint8).reshape(-1, 13), info)


def vertex_normals(px, py, pz, bc, kept):
    """(H, W, 3) f32: per vertex the f64 sum of (V1 - V0) x (V2 - V0) over its kept triangles -- quads (i - 1, j - 1), (i - 1, j), (i, j - 1), (i, j),
    T0 before T1 -- divided by its length; (0, 0, 0) where the length is zero or not finite (and at a vertex of no kept triangle)."""
    H, W = px.shape
    P = np.stack([px, py, pz], -1).astype(np.float64)
    A, B, C, D = P[:-1, :-1], P[:-1, 1:], P[1:, :-1], P[1:, 1:]
    sel = bc[..., None]

    def cross(v0, v1, v2):
        e, f = v1 - v0, v2 - v0
        return np.stack([e[..., 1] * f[..., 2] - e[..., 2] * f[..., 1], e[..., 2] * f[..., 0] - e[..., 0] * f[..., 2], e[..., 0] * f[..., 1] - e[..., 1] * f[..., 0]], -1)

    with np.errstate(all="ignore"):
        cr = [cross(A, C, np.where(sel, B, D)), cross(np.where(sel, B, A), np.where(sel, C, D), np.where(sel, D, B))]
    # does triangle t of a quad with diagonal b-c (bc) contain the corner?
    contains = {"a": (np.ones_like(bc), ~bc), "b": (bc, np.ones_like(bc)), "c": (np.ones_like(bc), bc), "d": (~bc, np.ones_like(bc))}
    # the vertex is corner d of quad (i - 1, j - 1), c of (i - 1, j), b of (i, j - 1), a of (i, j): where that corner sits in the (H, W) grid
    where = {"d": (slice(1, None), slice(1, None)), "c": (slice(1, None), slice(0, -1)), "b": (slice(0, -1), slice(1, None)), "a": (slice(0, -1), slice(0, -1))}
    N = np.zeros((H, W, 3), np.float64)
    for corner in ("d", "c", "b", "a"):
        for t in (0, 1):
            take = kept[..., t] & contains[corner][t]
            N[where[corner]] = N[where[corner]] + np.where(take[..., None], cr[t], 0.0)
    with np.errstate(all="ignore"):
        length = np.sqrt((N[..., 0] * N[..., 0] + N[..., 1] * N[..., 1]) + N[..., 2] * N[..., 2])
        ok = (length > 0) & np.isfinite(length)
        out = np.where(ok[..., None], (N / length[..., None]).astype(F32), F32(0))
    return out.astype(F32)


# ---- the input families ---------------------------------------------------------------------------------------------------------------------------
def plane(H, W):
    i, j = np.arange(H, dtype=np.float64).reshape(H, 1), np.arange(W, dtype=np.float64).reshape(1, W)
    return (20.0 * (1.0 + 0.01 * i + 0.002 * j)).astype(F32)


def family(name, H, W, focal=100.0, baseline=0.5):
    """dict(img (3, H, W) f32, disp (H, W) f32, focal, baseline, kw: the keyword arguments of build_ref / mesh.build beyond the camera)."""
    rng = np.random.default_rng([FAMILIES.index(name), H, W])
    img = (rng.random((3, H, W)) * 1.2 - 0.53).astype(F32)  # some colours below 0 and above 255
    kw = {}
    if name == "plane":
        disp = plane(H, W)
    elif name == "step":
        disp = plane(H, W)
        disp[:, W // 2:] *= F32(0.25)
    elif name == "holes":
        disp = plane(H, W)
        r = rng.random((H, W))
        disp[r < 0.15] = np.nan
        disp[(r >= 0.15) & (r < 0.20)] = -1.0
        disp[(r >= 0.20) & (r < 0.23)] = 0.1  # beyond max_depth
    elif name in ("random", "inf-jump"):
        disp = np.exp(rng.uniform(np.log(2.0), np.log(50.0), (H, W))).astype(F32)
        kw["max_jump"] = 0.5 if name == "random" else float("inf")
    elif name == "quant":
        disp = rng.choice(np.array([10.0, 10.4, 11.0, 30.0], F32), (H, W))
    elif name == "score":
        disp = plane(H, W)
        kw["score"], kw["threshold"] = rng.random((H, W), dtype=F32), 0.3
    else:
        raise ValueError(name)
    return dict(img=img, disp=np.ascontiguousarray(disp, F32), focal=focal, baseline=baseline, kw=kw)


# ---- a small PLY reader -----------------------------------------------------------------------------------------------------------------------------
def parse_ply(path):
    """-> (vertices: structured array with the header's property names, faces (nf, 3) int32, header: dict(format, vertex, face, properties))."""
    raw = open(path, "rb").read()
    end = raw.index(b"end_header\n") + len(b"end_header\n")
    lines = raw[:end].decode("ascii").splitlines()
    assert lines[0] == "ply"
    fmt = lines[1].split()[1]
    counts, props, element = {}, [], None
    for ln in lines[2:]:
        w = ln.split()
        if w[0] == "element":
            element = w[1]
            counts[element] = int(w[2])
        elif w[0] == "property" and element == "vertex":
            props.append((w[2], {"float": "<f4", "uchar": "u1"}[w[1]]))
        elif w[0] == "property":
            assert element == "face" and w[1:] == ["list", "uchar", "int", "vertex_indices"], ln
    nv, nf = counts["vertex"], counts.get("face", 0)
    dt = np.dtype(props)
    if fmt == "binary_little_endian":
        vert = np.frombuffer(raw, dt, nv, end)
        rec = np.frombuffer(raw, FACE, nf, end + nv * dt.itemsize)
        assert end + nv * dt.itemsize + nf * 13 == len(raw) and (rec["n"] == 3).all()
        faces = rec["v"].astype(np.int32)
    else:
        assert fmt == "ascii"
        body = raw[end:].decode("ascii").splitlines()
        assert len(body) == nv + nf
        vert = np.zeros(nv, dt)
        for k, ln in enumerate(body[:nv]):
            vert[k] = tuple(float(t) if p[1] == "<f4" else int(t) for t, p in zip(ln.split(), props))
        faces = np.array([[int(t) for t in ln.split()] for ln in body[nv:]], np.int32).reshape(-1, 4)
        assert (faces[:, 0] == 3).all()
        faces = faces[:, 1:]
    return vert, faces, dict(format=fmt, vertex=nv, face=nf, properties=[p[0] for p in props])
