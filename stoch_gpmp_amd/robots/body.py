"""The robot side of the voxel distance field: a body as collision spheres fixed in the link frames, each with its own radius
(include/sgpmp.h: SGPMP_COST_BODY_SDF, sgpmp_set_body) -- how GPMP2, CHOMP and cuRobo model an arm on a distance field.  No
reference counterpart.  Link frames are the FK chain's: frame 0 is the base, frame j + 1 follows joint j."""
from math import ceil, isfinite, sqrt

from .._lib import MAX_BODY


class BodySpheres:
    """`links[m]`, `centers[m]` (in that link's frame) and `radii[m]` of M spheres, 1 <= M <= 64.  The table is kept sorted by
    link (stably: spheres of one link keep their order), which is the order the kernels walk it in."""

    def __init__(self, links, centers, radii):
        links = [int(v) for v in links]
        centers = [tuple(float(c) for c in row) for row in centers]
        radii = [float(r) for r in radii]
        if not (len(links) == len(centers) == len(radii)) or not 1 <= len(links) <= MAX_BODY:
            raise ValueError(f"BodySpheres: links, centers and radii must have one entry per sphere, 1 to {MAX_BODY} spheres")
        if any(len(c) != 3 or not all(isfinite(v) for v in c) for c in centers):
            raise ValueError("BodySpheres: a centre is three finite numbers")
        if any(not isfinite(r) or r < 0. for r in radii):
            raise ValueError("BodySpheres: a radius must be finite and >= 0")
        if any(l < 0 for l in links):
            raise ValueError("BodySpheres: a link index must be >= 0")
        order = sorted(range(len(links)), key=lambda m: links[m])          # (sorted() is stable)
        self.links = tuple(links[m] for m in order)
        self.centers = tuple(centers[m] for m in order)
        self.radii = tuple(radii[m] for m in order)

    def __len__(self):
        return len(self.links)

    def __eq__(self, other):
        return isinstance(other, BodySpheres) and (self.links, self.centers, self.radii) == \
            (other.links, other.centers, other.radii)

    def __hash__(self):
        return hash((self.links, self.centers, self.radii))

    def table(self):
        """-> [M][4] rows (cx, cy, cz, r), the layout of sgpmp_set_body."""
        return [list(c) + [r] for c, r in zip(self.centers, self.radii)]

    def pair_rows(self, min_link_gap=2, ignore=()):
        """-> the rows of sgpmp_set_body_pairs, one int (uint64) per sphere: bit j of rows[i], j > i, is set where the spheres'
        link indices differ by at least `min_link_gap` and the link pair is not in `ignore` (pairs of link indices, in either
        order).  Neighbouring links touch at their joint by construction, hence the default gap of 2.  ValueError when nothing
        is counted (or when min_link_gap < 1: a pair on one link is a constant)."""
        from ..body_self import pair_rows                                   # (the numpy twin holds the rule)
        return pair_rows(self.links, min_link_gap, ignore)

    @classmethod
    def along_links(cls, chain, spacing, radius):
        """Spheres of one radius strung along the chain, from its constants alone: joint l (0-based), whose offset `xyz` is
        given in link l's frame, puts k = max(1, ceil(|xyz| / spacing)) spheres on link l at xyz * s / k, s = 0 .. k-1 -- from
        the link's origin towards the next joint -- and the last link gets one sphere at its origin.
        chain: list of (name, 'revolute'|'fixed', rpy, xyz)."""
        if not spacing > 0.:
            raise ValueError("BodySpheres.along_links: spacing must be > 0")
        links, centers = [], []
        for l, (_, _, _, xyz) in enumerate(chain):
            length = sqrt(sum(float(v) ** 2 for v in xyz))
            k = max(1, int(ceil(length / spacing)))
            for s in range(k):
                links.append(l)
                centers.append(tuple(float(v) * s / k for v in xyz))
        links.append(len(chain))
        centers.append((0., 0., 0.))
        return cls(links, centers, [radius] * len(links))
