"""3-D occupancy volume and its signed-distance field: the obstacle model of arm scenes beyond sphere lists (tables, shelves,
boxes, anything that arrives as an occupancy volume).  No reference counterpart.

`VoxelMap` holds the occupancy volume [nz, ny, nx] on the device; `VoxelDistanceField` is the hinge on its exact Euclidean
signed distance at the link points of an FK chain (include/sgpmp.h: SGPMP_COST_VOXEL_SDF), built on the device by
csrc/sdf.hip and evaluated by `voxel_sdf_field` (csrc/cost_device.h).  Host-side twin: stoch_gpmp_amd/voxel_sdf.py.
"""
from math import ceil

import numpy as np
import torch

from .. import _lib as L
from ..costs.fields import DistanceField, _linspace_alpha
from ..engine import Engine
from .sdf_field import DeviceSdf


class VoxelMap:
    """Occupancy volume over the box [lower_corner, lower_corner + map_dim] (world units, (x, y, z)) in cubic cells of
    `cell_size`; cell (k, j, i) of `occ` [nz, ny, nx] has its centre at lower_corner + (i + 0.5, j + 0.5, k + 0.5) * cell_size.
    The volume lives on the device; the add_* methods paint it there."""

    def __init__(self, map_dim, cell_size, lower_corner=(0., 0., 0.), tensor_args=None):
        if tensor_args is None:
            tensor_args = {'device': torch.device('cuda:0'), 'dtype': torch.float32}
        if not cell_size > 0 or len(map_dim) != 3 or len(lower_corner) != 3:
            raise ValueError("VoxelMap: map_dim and lower_corner are (x, y, z), cell_size > 0")
        self.tensor_args = tensor_args
        self.cell_size = float(cell_size)
        self.lower_corner = tuple(float(v) for v in lower_corner)
        nx, ny, nz = (int(ceil(float(d) / self.cell_size - 1e-9)) for d in map_dim)
        self._alloc(nz, ny, nx)

    def _alloc(self, nz, ny, nx):
        if not all(1 <= n <= 512 for n in (nz, ny, nx)):
            raise ValueError(f"VoxelMap: {nz} x {ny} x {nx} cells; every extent must be in [1, 512]")
        L.require_cuda(self.tensor_args)
        self.occ = torch.zeros(nz, ny, nx, **self.tensor_args)

    @classmethod
    def from_grid(cls, grid, cell_size, lower_corner=(0., 0., 0.), tensor_args=None):
        """Wrap an existing [nz, ny, nx] occupancy array (numpy or torch), e.g. a depth camera's volume."""
        g = torch.as_tensor(np.asarray(grid.detach().cpu() if torch.is_tensor(grid) else grid, dtype=np.float64))
        if g.dim() != 3:
            raise ValueError("VoxelMap.from_grid: the grid must be [nz, ny, nx]")
        vm = cls([g.shape[2] * cell_size, g.shape[1] * cell_size, g.shape[0] * cell_size], cell_size, lower_corner, tensor_args)
        if tuple(vm.occ.shape) != tuple(g.shape):             # (a cell size whose multiples round badly)
            vm._alloc(*g.shape)
        vm.occ.copy_(g.to(**vm.tensor_args))
        return vm

    @property
    def origin(self):
        """(ox, oy, oz): a point p has the fractional cell index p / cell_size + origin - 0.5 (the term's offsets)."""
        return tuple(-c / self.cell_size for c in self.lower_corner)

    def cell_centers(self, axis):
        """World coordinates of the cell centres along axis 0 (x), 1 (y) or 2 (z), on the device."""
        n = self.occ.shape[2 - axis]
        return self.lower_corner[axis] + (torch.arange(n, **self.tensor_args) + 0.5) * self.cell_size

    def _paint(self, inside):
        self.occ.masked_fill_(inside, 1.)
        return self

    def add_box(self, center, size):
        """Occupy every cell whose centre lies in the axis-aligned box of `size` (x, y, z) about `center`."""
        m = [((self.cell_centers(a) - float(center[a])).abs() <= 0.5 * float(size[a])) for a in range(3)]
        return self._paint(m[2][:, None, None] & m[1][None, :, None] & m[0][None, None, :])

    def add_sphere(self, center, radius):
        """Occupy every cell whose centre lies within `radius` of `center`."""
        d = [(self.cell_centers(a) - float(center[a])) ** 2 for a in range(3)]
        return self._paint(d[2][:, None, None] + d[1][None, :, None] + d[0][None, None, :] <= float(radius) ** 2)

    def distance_field(self, margin, threshold=0., **kwargs):
        """The smooth collision field of this volume: VoxelDistanceField(self, margin, threshold, ...)."""
        return VoxelDistanceField(self, margin, threshold=threshold, **kwargs)

    def body_field(self, body, margin, threshold=0., **kwargs):
        """The same field evaluated at a body's collision spheres (robots/body.py): BodyDistanceField(self, body, margin, ...)."""
        return BodyDistanceField(self, body, margin, threshold=threshold, **kwargs)


class VoxelDistanceField(DeviceSdf, DistanceField):
    """Hinge on a voxel signed-distance field, summed over the link points of the FK chain: f(q) = sum_p max(margin - d(p), 0),
    d the trilinear interpolation of the volume's exact Euclidean signed distance -- the GPMP obstacle field for scenes given as
    occupancy.  The point set is LinkDistanceField's (every link origin + `num_interpolate` points per link pair of
    `link_interpolate_range`).  Accepted by CostCollision(field=...) in StochGPMP and GPMP (with and without continuous-time
    factors); not evaluated by the dense-trajectory cost (`dense_cost=` of StochGPMP raises ValueError).  After painting the
    map, `update()` rebuilds the distance volume on the device."""
    works_on_frames = True           # compute_cost takes link frames [.., L, 4, 4]

    def __init__(self, voxel_map, margin, threshold=0., num_interpolate=0, link_interpolate_range=[5, 7], **kwargs):
        kwargs.setdefault("tensor_args", voxel_map.tensor_args)
        super().__init__(**kwargs)
        if not margin >= 0.:
            raise ValueError("VoxelDistanceField: margin must be >= 0")
        self.voxel_map = voxel_map
        self.margin = float(margin)
        self.threshold = float(threshold)
        self.num_interpolate = num_interpolate
        self.link_interpolate_range = link_interpolate_range
        self._build()

    def _build(self):
        self._rebuild("voxel_sdf_build", 1, self.voxel_map.occ.contiguous(), self.voxel_map.cell_size)
        self._engines = {}           # the query engines hold the old tensor (or a converted copy of it)

    def descriptor(self, sigma, distance=False):
        vm = self.voxel_map
        ox, oy, oz = vm.origin
        return dict(kind=L.COST_VOXEL_SDF, flags=L.FLAG_GRID_DISTANCE if distance else 0, sigma=sigma, sigma2=self.margin,
                    device_tensor=self.sdf, reserved=self.sdf.shape[0], dim0=self.sdf.shape[1], dim1=self.sdf.shape[2],
                    p0=vm.cell_size, p1=ox, p2=oy, dt=oz, num_interpolate=self.num_interpolate,
                    interp_lo=self.link_interpolate_range[0], interp_hi=self.link_interpolate_range[1],
                    alpha=_linspace_alpha(self.num_interpolate))

    def compute_cost(self, link_tensor, **kwargs):
        """Link frames [.., L, 4, 4] -> the field [..] (`field_eval_kernel`)."""
        shape = link_tensor.shape[:-3]
        frames = link_tensor.contiguous()
        return self._engine(frames.dtype, frames.device).field_eval(0, frames).reshape(shape)

    def _query(self, q, chain):
        n = sum(1 for j in chain if j[1] == "revolute")
        key = ("distance", q.dtype, str(q.device), id(chain))
        if key not in self._engines:
            eng = Engine(n, 2, 0, 1, tensor_args={"device": q.device, "dtype": q.dtype})
            eng.set_fk(chain)
            eng.set_costs([self.descriptor(1.0, distance=True)])
            self._engines[key] = eng
        return self._engines[key].field_grad(0, q.reshape(-1, n).contiguous())

    def compute_distance(self, q, chain, **kwargs):
        """Joint configurations q [.., n] -> min over the link points of the interpolated signed distance [..] (negative
        inside obstacles): the query flag of the term (`_query` also returns its gradient, through the first arg-min point)."""
        return self._query(q, chain)[0].reshape(q.shape[:-1])

    def compute_collision(self, q, chain, buffer=0., **kwargs):
        """Does any link point come closer than `buffer` to an occupied cell? -> bool [..]"""
        return self.compute_distance(q, chain) < buffer


class BodyDistanceField(VoxelDistanceField):
    """The voxel field at a BODY: collision spheres fixed in the link frames, each with its radius (robots/body.py: BodySpheres),
    f(q) = sum_m max(margin - (d(p_m) - r_m), 0) with p_m = P_l + R_l c_m (include/sgpmp.h: SGPMP_COST_BODY_SDF) -- link
    geometry with thickness, where VoxelDistanceField sees link origins.  The volume, its rebuild, `update()` and
    `compute_collision` are VoxelDistanceField's; the point set is the body's (no interpolated points).  Accepted by
    CostCollision(field=...) in StochGPMP and GPMP (with and without continuous-time factors); not evaluated by the
    dense-trajectory cost (`dense_cost=` of StochGPMP raises ValueError)."""

    def __init__(self, voxel_map, body, margin, threshold=0., **kwargs):
        if not len(body):
            raise ValueError("BodyDistanceField: the body has no spheres")
        self.body = body
        super().__init__(voxel_map, margin, threshold=threshold, num_interpolate=0, **kwargs)

    def descriptor(self, sigma, distance=False):
        return dict(super().descriptor(sigma, distance=distance), kind=L.COST_BODY_SDF, body=self.body)

    def compute_cost(self, link_tensor, **kwargs):
        """Link frames [.., L, 4, 4] -> the field [..] (`body_eval_kernel`).  The frames carry the rotations and sgpmp_field_eval
        checks the body's last link against L; the context needs a chain only because sgpmp_set_body checks the link indices
        against one: a placeholder with as many frames as the body reaches."""
        shape = link_tensor.shape[:-3]
        frames = link_tensor.contiguous()
        key = ("frames", frames.dtype, str(frames.device))
        if key not in self._engines:
            eng = Engine(1, 2, 0, 1, tensor_args={"device": frames.device, "dtype": frames.dtype})
            eng.set_fk([("placeholder", "revolute" if j == 0 else "fixed", (0., 0., 0.), (0., 0., 0.))
                        for j in range(max(self.body.links[-1], 1))], codegen=False)
            eng.set_costs([self.descriptor(1.0)])
            self._engines[key] = eng
        return self._engines[key].field_eval(0, frames).reshape(shape)

    def _query(self, q, chain, distance=True):
        n = sum(1 for j in chain if j[1] == "revolute")
        key = ("distance" if distance else "grad", q.dtype, str(q.device), id(chain))
        if key not in self._engines:
            eng = Engine(n, 2, 0, 1, tensor_args={"device": q.device, "dtype": q.dtype})
            eng.set_fk(chain, codegen=False)
            eng.set_costs([self.descriptor(1.0, distance=distance)])
            self._engines[key] = eng
        return self._engines[key].field_grad(0, q.reshape(-1, n).contiguous())

    def compute_cost_and_grad(self, q, chain, **observations):
        """Field value [B] and gradient [B, n] at joint configurations q [B, n] (`body_grad_kernel`)."""
        return self._query(q, chain, distance=False)

    def compute_distance(self, q, chain, **kwargs):
        """Joint configurations q [.., n] -> the body's minimum clearance min_m (d(p_m) - r_m) [..] (negative in collision): the
        query flag of the term (`_query` also returns its gradient, through the first arg-min sphere)."""
        return self._query(q, chain)[0].reshape(q.shape[:-1])
