from .cheb import ChebCovariance, cheb_eval, cheb_fit, matern_density, matern_density_grad, trimesh_lbo_fem, trimesh_lbo_fem_mass  # noqa: F401
from .operator import ChebCovCondition, CovCondition  # noqa: F401
from .streamer_build import DeviceSvdFactorizer, densify, stream_butterfly, truncated_svd_device  # noqa: F401
