"""Host side of the field statistics (no GPU): the VTK writers of multigridmc_amd.vtk against the format of
VTKWriter2d / VTKWriter3d::write and write_vtk_circle (auxilliary/vtk_writer2d.cc, vtk_writer3d.cc), built
here line by line, and the NULL-handle contract of the mgmc_field_stats_* entry points."""
import ctypes

import numpy as np

import multigridmc_amd as mg
from multigridmc_amd import _native


def _expected(shape, fields):
    """the file, point by point, as the format is stated"""
    dim = len(shape)
    n = list(shape) + [0] * (3 - dim)
    lines = ["# vtk DataFile Version 2.0", "Sample state", "ASCII", "DATASET STRUCTURED_POINTS"]
    if dim == 2:
        lines += ["DIMENSIONS %d %d 1 " % (n[0] + 1, n[1] + 1), "ORIGIN -0.5 -0.5 0.0",
                  "SPACING %g %g 0" % (1.0 / n[0], 1.0 / n[1])]
    else:
        lines += ["DIMENSIONS %d %d %d" % (n[0] + 1, n[1] + 1, n[2] + 1), "ORIGIN -0.5 -0.5 -5.0",
                  "SPACING %g %g %g" % (1.0 / n[0], 1.0 / n[1], 1.0 / n[2])]
    npts = (n[0] + 1) * (n[1] + 1) * (n[2] + 1 if dim == 3 else 1)
    lines += ["", "POINT_DATA %d" % npts]
    for label in sorted(fields):
        phi = fields[label]
        lines += ["SCALARS %s double 1" % label, "LOOKUP_TABLE default"]
        count = 0
        for k in range(n[2] + 1 if dim == 3 else 1):
            for j in range(n[1] + 1):
                for i in range(n[0] + 1):
                    data = 0.0
                    inside = 0 < i < n[0] and 0 < j < n[1] and (dim == 2 or 0 < k < n[2])
                    if inside:
                        idx = (i - 1) + (n[0] - 1) * (j - 1) + ((n[0] - 1) * (n[1] - 1) * (k - 1) if dim == 3 else 0)
                        data = phi[idx]
                        if abs(data) < 1.0e-20:
                            data = 0.0
                    lines.append("%g" % data)
                    count += 1
        assert count == npts
    return "\n".join(lines) + "\n"


def _fields(ndof):
    rng = np.random.default_rng(3)
    mean = rng.standard_normal(ndof)
    mean[1] = 3.0e-21      # below 1e-20: written as 0
    mean[2] = -7.0e-23
    mean[3] = 1.5e-20      # not below: stays, exponent form
    variance = rng.random(ndof) + 0.5
    variance[0] = 1.234567891e-7   # %g exponent form, 6 significant digits
    variance[4] = 2.5e12
    exact = np.arange(ndof, dtype=np.float64) / 8.0
    return {"mean": mean, "variance": variance, "mean_exact": exact}


def _check(tmp_path, shape):
    lat = mg.Lattice(*shape)
    fields = _fields(lat.Nvertex)
    path = tmp_path / "out.vtk"
    mg.write_vtk(str(path), lat, fields)
    text = path.read_text()
    assert text == _expected(shape, fields)
    lines = text.split("\n")
    npts = int(np.prod([n + 1 for n in shape]))
    assert [ln.split()[1] for ln in lines if ln.startswith("SCALARS")] == ["mean", "mean_exact", "variance"]
    assert len(lines) - 1 == 9 + 3 * (2 + npts)
    first = lines.index("SCALARS mean double 1") + 2
    values = lines[first:first + npts]
    assert "1.5e-20" in values and "3e-21" not in values and "-7e-23" not in values
    assert "1.23457e-07" in lines and "2.5e+12" in lines
    return lines


def test_write_vtk_2d(tmp_path):
    lines = _check(tmp_path, (4, 4))
    assert lines[4] == "DIMENSIONS 5 5 1 "  # the reference's trailing blank
    assert lines[5] == "ORIGIN -0.5 -0.5 0.0" and lines[6] == "SPACING 0.25 0.25 0"
    assert lines[7] == "" and lines[8] == "POINT_DATA 25"


def test_write_vtk_3d(tmp_path):
    lines = _check(tmp_path, (4, 4, 4))
    assert lines[4] == "DIMENSIONS 5 5 5"
    assert lines[5] == "ORIGIN -0.5 -0.5 -5.0" and lines[6] == "SPACING 0.25 0.25 0.25"
    assert lines[8] == "POINT_DATA 125"


def test_write_vtk_rectangular_lattice_x_fastest(tmp_path):
    lat = mg.Lattice(4, 3)
    phi = np.arange(1.0, lat.Nvertex + 1)  # 3 x 2 interior vertices
    mg.write_vtk(str(tmp_path / "r.vtk"), lat, {"phi": phi})
    assert (tmp_path / "r.vtk").read_text() == _expected((4, 3), {"phi": phi})


def test_write_vtk_circle(tmp_path):
    path = tmp_path / "circle.vtk"
    mg.write_vtk_circle([0.5, 0.25], 0.1, str(path))
    lines = path.read_text().split("\n")
    assert lines[:6] == ["# vtk DataFile Version 2.0", "Sample state", "ASCII", "DATASET POLYDATA", "",
                         "POINTS 100 double"]
    pts = lines[6:106]
    for j, ln in enumerate(pts):
        x = 0.5 + 0.1 * np.cos(2 * np.pi * j / 100.0) - 0.5
        y = 0.25 + 0.1 * np.sin(2 * np.pi * j / 100.0) - 0.5
        assert ln == "%g %g %g" % (x, y, 1.0e-6)
    assert lines[106] == "POLYGONS 1 101"
    assert lines[107] == " ".join(["100"] + [str(j) for j in range(100)])
    assert lines[108:] == [""]


def test_field_stats_entry_points_reject_a_null_handle():
    lib = mg.load_library()
    en, st, n = ctypes.c_int(), ctypes.c_int(), ctypes.c_uint64()
    buf = np.zeros(4)
    p = buf.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    assert lib.mgmc_field_stats_enable(None, 1) == _native.MGMC_E_INVALID
    assert lib.mgmc_field_stats_disable(None) == _native.MGMC_E_INVALID
    assert lib.mgmc_field_stats_reset(None) == _native.MGMC_E_INVALID
    assert lib.mgmc_field_stats_info(None, ctypes.byref(en), ctypes.byref(st), ctypes.byref(n)) == _native.MGMC_E_INVALID
    assert lib.mgmc_field_stats_get(None, p, p, 4) == _native.MGMC_E_INVALID
    assert "null handle" in _native.last_error()
