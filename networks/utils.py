from accflow_amd.networks.utils import backwarp, coords_grid, forward_interpolate  # noqa: F401
