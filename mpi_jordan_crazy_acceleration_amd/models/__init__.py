"""Solver "models": the block Gauss-Jordan inverter and the linear-system solver built on it."""
from .gauss_jordan import (Factored, GaussJordan, SingularMatrixError, factor, inverse, run,  # noqa: F401
                           solve)
