"""qamreconciliation.density_evolution: sampled density evolution of a code ensemble on the LAPPRs, which
the reference does not have (qamr.density_evolution)."""
from qamr.density_evolution import (DEResult, DETables, degree_tables, evolve, evolve_device,  # noqa: F401
                                    signed_population)

__all__ = ["degree_tables", "DETables", "DEResult", "signed_population", "evolve_device", "evolve"]
