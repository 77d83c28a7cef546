"""What the two signed-distance field objects share (GridDistanceField in obst_map.py, VoxelDistanceField in voxel_map.py): the
distance tensor `sdf`, built on the device from the map's occupancy and rebuilt in place where shape, dtype and device allow,
and `update()`, whose version bump makes the planners holding the field re-compile their cost program."""
from ..engine import Engine


class DeviceSdf:
    """Mixin; the field keeps `threshold` and `_version`, and its `_build()` calls `_rebuild` on the map's occupancy."""
    sdf = None
    _build_engine = None             # (key, Engine): one context for every rebuild

    def _rebuild(self, build, n_dof, occ, cell):
        """self.sdf = Engine.`build`(occ, cell, self.threshold), through a context of occ's dtype and device.  -> was it in
        place (then engines that hold the tensor itself, not a converted copy, are still valid)?"""
        key = (occ.dtype, str(occ.device))
        if self._build_engine is None or self._build_engine[0] != key:
            self._build_engine = (key, Engine(n_dof, 2, 0, 1, tensor_args={"device": occ.device, "dtype": occ.dtype}))
        in_place = self.sdf is not None and self.sdf.shape == occ.shape and self.sdf.dtype == occ.dtype and \
            self.sdf.device == occ.device
        self.sdf = getattr(self._build_engine[1], build)(occ, cell, self.threshold, out=self.sdf if in_place else None)
        return in_place

    def update(self):
        """Rebuild the distance field from the map's current occupancy (stream-ordered launches) and tell every planner
        holding this field to re-compile its cost program before its next step."""
        self._build()
        self._version += 1
        return self.sdf
