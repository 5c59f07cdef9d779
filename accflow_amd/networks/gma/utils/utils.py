from ...raft.utils.utils import backwarp, coords_grid, forward_interpolate  # noqa: F401
