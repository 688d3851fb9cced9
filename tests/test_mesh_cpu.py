"""CPU: the pinned surface-nets algorithm as restated in numpy (tests/support/surface_nets_ref.py, the reference the HIP
extractor is compared with bit for bit in tests/test_gpu_mesh.py) makes closed, outward-oriented meshes of the right
topology and size on analytic shapes; the PLY writer and reader of holo_diffusion_amd/mesh.py."""
import math

import numpy as np
import pytest

from holo_diffusion_amd import mesh
from tests.support import surface_nets_ref as ref

H, M = 3.5, 20  # (at m = 12 the torus below has edges shared by four triangles: the lattice is too coarse for its hole)
SPACING = 2 * H / (M - 1)
OFFSET = math.sqrt(3.0) * SPACING  # a cell's diagonal
CENTRE = np.array([0.3, -0.2, 0.45])


def lattice(m=M, h=H):
    g = np.linspace(-h, h, m)
    return np.meshgrid(g, g, g, indexing="ij")  # Z, Y, X


def sphere_volume(r):
    return 4.0 / 3.0 * math.pi * r ** 3


def analytic_cases():
    Z, Y, X = lattice()
    x, y, z = X - CENTRE[0], Y - CENTRE[1], Z - CENTRE[2]
    torus_volume = lambda r: 2 * math.pi ** 2 * 1.9 * r ** 2  # noqa: E731
    two = np.maximum(1.0 - np.sqrt((X + 1.7) ** 2 + Y ** 2 + Z ** 2), 0.9 - np.sqrt((X - 1.6) ** 2 + (Y - 0.3) ** 2 + Z ** 2))
    return {
        # name: (field, Euler characteristic, volume of the shape offset by d)
        "sphere": (2.1 - np.sqrt(x ** 2 + y ** 2 + z ** 2), 2, lambda d: sphere_volume(2.1 + d)),
        "torus": (0.8 - np.sqrt((np.sqrt(x ** 2 + y ** 2) - 1.9) ** 2 + z ** 2), 0, lambda d: torus_volume(0.8 + d)),
        "two spheres": (two, 4, lambda d: sphere_volume(1.0 + d) + sphere_volume(0.9 + d)),
        "all inside": (np.ones_like(X), 2, lambda d: (2 * (H + d)) ** 3),
    }


@pytest.fixture(scope="module")
def meshes():
    return {name: ref.surface_nets(field, 0.0, H) + (chi, vol) for name, (field, chi, vol) in analytic_cases().items()}


@pytest.mark.parametrize("name", ["sphere", "torus", "two spheres", "all inside"])
def test_analytic_shapes_are_closed_oriented_and_sized(meshes, name):
    verts, faces, chi, volume = meshes[name]
    assert verts.dtype == np.float32 and faces.dtype == np.int32 and faces.min() >= 0 and faces.max() < len(verts)
    assert ref.euler_characteristic(verts, faces) == chi
    assert (ref.edge_use(faces)[1] == 2).all()  # a closed 2-manifold: every edge between exactly two triangles
    vol = ref.signed_volume(verts, faces)  # positive: the triangles face outward
    assert 0.0 < volume(-OFFSET) < vol < volume(OFFSET), (vol, volume(-OFFSET), volume(OFFSET))


def test_sphere_vertices_lie_in_cells_the_surface_crosses(meshes):
    verts = meshes["sphere"][0]
    dist = np.abs(np.linalg.norm(verts.astype(np.float64) - CENTRE, axis=1) - 2.1)
    assert dist.max() <= OFFSET


def test_white_noise_mesh_is_closed():
    """Every cell is active and some edges carry four triangles (the surface touches itself there): the count per edge
    is even, not two."""
    verts, faces = ref.surface_nets(np.random.default_rng(0).standard_normal((9, 9, 9)), 0.0, H)
    use = ref.edge_use(faces)[1]
    assert len(verts) > 0.9 * 6 ** 3 and (use % 2 == 0).all() and (use == 4).any()


def test_degenerate_lattices():
    for field in (np.ones((2, 2, 2)), -np.ones((7, 7, 7))):  # m = 2 has no interior; all outside
        verts, faces = ref.surface_nets(field, 0.0, 1.0)
        assert verts.shape == (0, 3) and faces.shape == (0, 3)
    cube = -np.ones((3, 3, 3))
    cube[1, 1, 1] = 1.0
    verts, faces = ref.surface_nets(cube, 0.0, 1.0)
    assert verts.shape == (8, 3) and faces.shape == (12, 3)
    # each corner cell averages three crossings, half way along the three edges into the centre: (5/6) * spacing - h
    assert np.allclose(np.abs(verts), 1.0 / 6.0, rtol=0, atol=1e-6)
    assert ref.signed_volume(verts, faces) == pytest.approx(1.0 / 27.0, rel=1e-5)
    # a value equal to the level is outside
    cube[1, 1, 1] = 0.0
    assert ref.surface_nets(cube, 0.0, 1.0)[0].shape == (0, 3)


def test_ply_round_trip(tmp_path):
    verts, faces = meshes_for_ply()
    rng = np.random.default_rng(5)
    normals = rng.standard_normal(verts.shape).astype(np.float32)
    colours = (rng.integers(0, 256, verts.shape).astype(np.float32) / np.float32(255.0))
    path = mesh.save_ply(str(tmp_path / "mesh.ply"), verts, faces, normals, colours)
    raw = open(path, "rb").read()
    # the header, by hand
    head, _, body = raw.partition(b"end_header\n")
    lines = head.decode("ascii").splitlines()
    assert lines[:2] == ["ply", "format binary_little_endian 1.0"]
    props = [ln for ln in lines if ln.startswith(("element", "property"))]
    assert props == [f"element vertex {len(verts)}"] + [f"property float {n}" for n in ("x", "y", "z", "nx", "ny", "nz")] + \
        [f"property uchar {n}" for n in ("red", "green", "blue")] + \
        [f"element face {len(faces)}", "property list uchar int vertex_indices"]
    assert len(body) == len(verts) * (6 * 4 + 3) + len(faces) * (1 + 3 * 4)
    assert np.array_equal(np.frombuffer(body[:12], "<f4"), verts[0])
    first_face = body[len(verts) * 27:][:13]
    assert first_face[0] == 3 and np.array_equal(np.frombuffer(first_face[1:], "<i4"), faces[0])
    back = mesh.load_ply(path)
    assert np.array_equal(back["verts"], verts) and np.array_equal(back["faces"], faces)
    assert np.array_equal(back["normals"], normals) and np.array_equal(back["colours"], colours)
    assert back["verts"].dtype == np.float32 and back["faces"].dtype == np.int32
    # an empty mesh, and defaults for missing attributes
    empty = mesh.load_ply(mesh.save_ply(str(tmp_path / "empty.ply"), np.zeros((0, 3)), np.zeros((0, 3))))
    assert empty["verts"].shape == (0, 3) and empty["faces"].shape == (0, 3)
    bare = mesh.load_ply(mesh.save_ply(str(tmp_path / "bare.ply"), verts, faces))
    assert not bare["normals"].any() and np.array_equal(bare["faces"], faces)
    with pytest.raises(ValueError, match="past the vertices"):
        mesh.save_ply(str(tmp_path / "bad.ply"), verts[:3], faces)
    (tmp_path / "cut.ply").write_bytes(raw[:-5])
    with pytest.raises(ValueError, match="truncated"):
        mesh.load_ply(str(tmp_path / "cut.ply"))


def meshes_for_ply():
    Z, Y, X = lattice(8)
    return ref.surface_nets(2.1 - np.sqrt(X ** 2 + Y ** 2 + Z ** 2), 0.0, H)


def test_default_density_level_and_half_extent():
    # one voxel's length of material at this density is `opacity_level` opaque
    for voxel, opacity in ((1.0, 0.5), (0.125, 0.5), (0.25, 0.9)):
        level = mesh.default_density_level(voxel, opacity)
        assert 1.0 - math.exp(-level * voxel) == pytest.approx(opacity, rel=1e-12)
    assert mesh.default_density_level(1.0) == pytest.approx(math.log(2.0))
    with pytest.raises(ValueError):
        mesh.default_density_level(1.0, 1.0)
    assert mesh.half_extent(8, 8.0) == 3.5 and mesh.half_extent(64, 8.0) == pytest.approx(63 / 64 * 4.0, rel=1e-6)


def test_generate_cli_mesh_keys(tmp_path):
    """save_mesh / mesh_resolution / mesh_opacity_level: off by default (no file, no extract_mesh call); on, every sample
    lands as sample_%05d_mesh.ply next to the frames with the model's mesh in it."""
    import torch

    from holo_diffusion_amd import generate

    cfg = generate.parse_cli(["exp_dir=x"])
    assert (cfg["save_mesh"], cfg["mesh_resolution"], cfg["mesh_opacity_level"]) == (False, None, 0.5)
    cfg = generate.parse_cli(["exp_dir=x", "save_mesh=true", "mesh_resolution=33", "mesh_opacity_level=0.25"])
    assert (cfg["save_mesh"], cfg["mesh_resolution"], cfg["mesh_opacity_level"]) == (True, 33, 0.25)
    for bad in ("save_mesh=3", "mesh_resolution=1", "mesh_resolution=1025", "mesh_opacity_level=1.0", "mesh_opacity_level=0"):
        with pytest.raises(SystemExit):
            generate.parse_cli(["exp_dir=x", bad])

    verts, faces = meshes_for_ply()
    calls = []

    class Model(torch.nn.Module):
        net_3d_enabled = diffusion_enabled = True
        render_image_width = render_image_height = 4

        def sample_random_voxel_features(self, **kw):
            return torch.randn(1, 4, 2, 2, 2)

        def render_views(self, vf, cams):
            img = vf.mean() + torch.zeros(len(cams), 3, 4, 4)
            return {"images_render": img, "depths_render": img[:, :1], "masks_render": img[:, :1]}

        def extract_mesh(self, vf, resolution=None, opacity_level=0.5):
            calls.append((float(vf.mean()), resolution, opacity_level))
            v = torch.from_numpy(verts) + float(vf.mean())
            return {"verts": v, "faces": torch.from_numpy(faces), "normals": torch.zeros_like(v),
                    "colours": torch.full_like(v, 0.2), "density_level": 1.0}

    load_fn = lambda exp_dir, render_size=None, device=None: (Model(), "report")  # noqa: E731
    run = lambda out_dir, **kw: generate.generate_samples_from_experiment(  # noqa: E731
        "exp", output_directory=str(out_dir), n_eval_cameras=2, num_samples=2, device=torch.device("cpu"), load_fn=load_fn, **kw)
    out = run(tmp_path / "plain")
    assert not calls and "meshes" not in out and not list((tmp_path / "plain").glob("*.ply"))
    out = run(tmp_path / "meshed", save_mesh=True, mesh_resolution=9, mesh_opacity_level=0.3)
    assert [c[1:] for c in calls] == [(9, 0.3)] * 2 and sorted(out["meshes"]) == [0, 1]
    for i in range(2):
        back = mesh.load_ply(str(tmp_path / "meshed" / f"sample_{i:05d}_mesh.ply"))
        assert np.array_equal(back["faces"], faces) and np.allclose(back["verts"], verts + calls[i][0], atol=1e-6)
        assert (tmp_path / "meshed" / f"sample_{i:05d}_frames.pt").exists()
    # the reference's call form: <sequence>_mesh.ply beside <sequence>_voxel_features.pth
    calls.clear()
    generate.render_flyaround(None, "seq7", Model(), str(tmp_path / "fly" / "video.mp4"), n_flyaround_poses=2,
                              trajectory_type="simple_360", device="cpu", sample_mode=True, save_voxel_features=True,
                              save_mesh=True, mesh_resolution=11)
    assert (tmp_path / "fly" / "seq7_voxel_features.pth").exists() and [c[1:] for c in calls] == [(11, 0.5)]
    assert np.array_equal(mesh.load_ply(str(tmp_path / "fly" / "seq7_mesh.ply"))["faces"], faces)
