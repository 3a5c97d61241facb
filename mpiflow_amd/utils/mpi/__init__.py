"""The utils/mpi drop-ins.  plane_geometry_grad(): the context manager that opens the gradients of the plane geometry."""
from ._autograd import plane_geometry_grad  # noqa: F401
