"""qamreconciliation.mutual_information (mutual_information.pyx): the names the reference's
sims/sim_montecarlo_information.py imports, plus the closed-form I(X;Xhat).  The quad-integrated
evaluators (mutual_information_base_scheme, mutual_information_X_Y and their integrands) are out
of scope of the MI355X build."""
from qamr.mutual_information import P_xhat, montecarlo_information, mutual_information_X_Xhat  # noqa: F401

__all__ = ["P_xhat", "montecarlo_information", "mutual_information_X_Xhat"]
