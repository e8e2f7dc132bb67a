"""Legacy-VTK output of lattice fields, in the format of the reference's VTKWriter2d / VTKWriter3d
(auxilliary/vtk_writer2d.cc:8-53, vtk_writer3d.cc:8-58) and write_vtk_circle (vtk_writer2d.cc:56-84).

A structured-points file over all (n+1)^d lattice points:

    # vtk DataFile Version 2.0
    Sample state
    ASCII
    DATASET STRUCTURED_POINTS
    DIMENSIONS <nx+1> <ny+1> 1             (2D, followed by one blank)    |  DIMENSIONS <nx+1> <ny+1> <nz+1>
    ORIGIN -0.5 -0.5 0.0                   (2D)                           |  ORIGIN -0.5 -0.5 -5.0
    SPACING <1/nx> <1/ny> 0                (2D)                           |  SPACING <1/nx> <1/ny> <1/nz>
    <empty line>
    POINT_DATA <number of points>

then, for every field in ascending order of its label (the reference keeps them in a std::map),

    SCALARS <label> double 1
    LOOKUP_TABLE default

and one value per line with x fastest: 0 on the boundary, the field's value at interior vertices, values
of magnitude below 1e-20 as 0.  Numbers are printed as a C++ ostream prints a double: printf's %g.
"""
from __future__ import annotations

import numpy as np

__all__ = ["write_vtk", "write_vtk_circle"]


def _g(v) -> str:
    return "%g" % v


def write_vtk(filename, lattice, fields) -> None:
    """Write `fields` ({label: vector over the interior vertices, x fastest}) on `lattice` (a Lattice, or
    its shape) to `filename`."""
    shape = tuple(int(v) for v in getattr(lattice, "shape", lattice))
    dim = len(shape)
    if dim not in (2, 3):
        raise ValueError("lattice must be 2D or 3D")
    npoints = int(np.prod([n + 1 for n in shape]))
    ninterior = int(np.prod([n - 1 for n in shape]))
    head = ["# vtk DataFile Version 2.0", "Sample state", "ASCII", "DATASET STRUCTURED_POINTS"]
    if dim == 2:
        head += [f"DIMENSIONS {shape[0] + 1} {shape[1] + 1} 1 ", "ORIGIN -0.5 -0.5 0.0",
                 f"SPACING {_g(1.0 / shape[0])} {_g(1.0 / shape[1])} 0"]
    else:
        head += [f"DIMENSIONS {shape[0] + 1} {shape[1] + 1} {shape[2] + 1}", "ORIGIN -0.5 -0.5 -5.0",
                 f"SPACING {_g(1.0 / shape[0])} {_g(1.0 / shape[1])} {_g(1.0 / shape[2])}"]
    head += ["", f"POINT_DATA {npoints}"]
    interior = tuple(slice(1, n) for n in reversed(shape))  # arrays are indexed [z,] y, x
    with open(filename, "w") as out:
        out.write("\n".join(head) + "\n")
        for label in sorted(fields):
            phi = np.asarray(fields[label], dtype=np.float64).reshape(-1)
            if phi.size != ninterior:
                raise ValueError(f"field '{label}' has {phi.size} values, the lattice {ninterior} interior vertices")
            full = np.zeros(tuple(n + 1 for n in reversed(shape)))
            full[interior] = np.where(np.abs(phi) < 1.0e-20, 0.0, phi).reshape(tuple(n - 1 for n in reversed(shape)))
            out.write(f"SCALARS {label} double 1\nLOOKUP_TABLE default\n")
            out.write("\n".join(np.char.mod("%g", full.reshape(-1))) + "\n")


def write_vtk_circle(centre, radius, filename) -> None:
    """A 100-gon around `centre` (unit-square coordinates) of the given radius as VTK polydata, shifted
    by the lattice origin (-0.5, -0.5) and lifted by 1e-6 (vtk_writer2d.cc:56-84)."""
    npoints = 100
    j = np.arange(npoints)
    x = float(centre[0]) + float(radius) * np.cos(2 * np.pi * j / (1.0 * npoints)) - 0.5
    y = float(centre[1]) + float(radius) * np.sin(2 * np.pi * j / (1.0 * npoints)) - 0.5
    rows = np.char.add(np.char.add(np.char.mod("%g", x), " "), np.char.mod("%g", y))
    with open(filename, "w") as out:
        out.write("# vtk DataFile Version 2.0\nSample state\nASCII\nDATASET POLYDATA\n\n")
        out.write(f"POINTS {npoints} double\n")
        out.write("\n".join(r + " " + _g(1.0e-6) for r in rows) + "\n")
        out.write(f"POLYGONS 1 {npoints + 1}\n")
        out.write(" ".join([str(npoints)] + [str(v) for v in j]) + "\n")
