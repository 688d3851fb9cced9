"""Surface nets as include/holo_abi.h pins them, restated in vectorised numpy (float32, one rounding per operation), plus
the mesh measures the tests assert on.  The HIP passes (kernels_mesh.hip) must agree with ``surface_nets`` bit for bit."""
import numpy as np

QUAD_OFFSETS = ((-1, -1), (0, -1), (0, 0), (-1, 0))


def lattice_spacing(half_extent, m):
    """2h / (m - 1) from the float32 half extent, rounded once from double."""
    return np.float32(2.0 * float(np.float32(half_extent)) / (m - 1))


def lattice_axis(half_extent, m):
    """float32 world coordinate of every index of one axis: (float)i * spacing - h."""
    return np.arange(m, dtype=np.float32) * lattice_spacing(half_extent, m) - np.float32(half_extent)


def _corner(a, c, dx, dy, dz):
    return a[dz:dz + c, dy:dy + c, dx:dx + c]


def surface_nets(field, level, half_extent):
    """field (m, m, m) indexed [z][y][x] -> verts (V, 3) float32, faces (F, 3) int32."""
    f = np.array(field, dtype=np.float32, copy=True)
    m = f.shape[0]
    assert f.shape == (m, m, m) and m >= 2
    lv, h, s = np.float32(level), np.float32(half_extent), lattice_spacing(half_extent, m)
    edge = np.zeros(f.shape, bool)
    edge[[0, -1]] = edge[:, [0, -1]] = edge[:, :, [0, -1]] = True
    f[edge] = lv - np.abs(f[edge] - lv)  # the boundary is never inside
    ins = f > lv
    c = m - 1
    n_in = sum(_corner(ins, c, dx, dy, dz).astype(np.int32) for dz in (0, 1) for dy in (0, 1) for dx in (0, 1))
    active = (n_in > 0) & (n_in < 8)
    acc = np.zeros((3, c, c, c), np.float32)
    cnt = np.zeros((c, c, c), np.int32)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        for ax in range(3):
            au, av = (ax + 1) % 3, (ax + 2) % 3
            for u in (0, 1):
                for v in (0, 1):
                    a = [0, 0, 0]
                    a[au], a[av] = u, v
                    b = list(a)
                    b[ax] = 1
                    fa, fb = _corner(f, c, *a), _corner(f, c, *b)
                    cross = _corner(ins, c, *a) != _corner(ins, c, *b)
                    p = [np.float32(a[0]), np.float32(a[1]), np.float32(a[2])]
                    p[ax] = (fa - lv) / (fa - fb)
                    for d in range(3):
                        acc[d] = np.where(cross, acc[d] + p[d], acc[d])
                    cnt += cross
    kk, jj, ii = np.nonzero(active)  # C order = increasing cell linear index
    n = cnt[kk, jj, ii].astype(np.float32)
    idx = (ii, jj, kk)
    verts = np.stack([(idx[d].astype(np.float32) + acc[d][kk, jj, ii] / n) * s - h for d in range(3)], axis=1)
    verts = verts.astype(np.float32).reshape(-1, 3)
    cid = -np.ones((c, c, c), np.int64)
    cid[kk, jj, ii] = np.arange(len(kk))
    keys, quads = [], []
    for ax in range(3):
        au, av = (ax + 1) % 3, (ax + 2) % 3
        lo, hi = [slice(None)] * 3, [slice(None)] * 3
        lo[2 - ax], hi[2 - ax] = slice(0, m - 1), slice(1, m)
        pk, pj, pi = np.nonzero(ins[tuple(lo)] != ins[tuple(hi)])  # the edge's first endpoint
        p = np.stack([pi, pj, pk])
        cells = []
        for du, dv in QUAD_OFFSETS:
            q = p.copy()
            q[au] += du
            q[av] += dv
            assert (q >= 0).all() and (q < c).all()
            cells.append(cid[q[2], q[1], q[0]])
        q4 = np.stack(cells, axis=1).reshape(-1, 4)
        assert (q4 >= 0).all()
        q4 = np.where(ins[pk, pj, pi][:, None], q4, q4[:, ::-1])  # normals from inside to outside
        keys.append(((pk * m + pj) * m + pi) * 3 + ax)
        quads.append(q4)
    q4 = np.concatenate(quads)[np.argsort(np.concatenate(keys), kind="stable")]
    faces = np.stack([q4[:, [0, 1, 2]], q4[:, [0, 2, 3]]], axis=1).reshape(-1, 3).astype(np.int32)
    return verts, faces


def edge_use(faces):
    """(unique undirected edges, number of triangles on each)."""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    e.sort(axis=1)
    if len(e) == 0:
        return e, np.zeros(0, np.int64)
    return np.unique(e, axis=0, return_counts=True)


def euler_characteristic(verts, faces):
    return len(verts) - len(edge_use(faces)[0]) + len(faces)


def signed_volume(verts, faces):
    v = np.asarray(verts, np.float64)
    a, b, c = v[faces[:, 0]], v[faces[:, 1]], v[faces[:, 2]]
    return float((a * np.cross(b, c)).sum() / 6.0)
