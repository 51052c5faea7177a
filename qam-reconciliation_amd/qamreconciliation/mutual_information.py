"""qamreconciliation.mutual_information (mutual_information.pyx): the names the reference's
sims/sim_montecarlo_information.py, sims/sim_mutual_information_base_scheme.py and
sims/sim_mutual_information_compare_signs.py import, plus the two integrands; and the LAPPR
information rate, which the reference does not have."""
from qamr.mutual_information import (P_xhat, lappr_information, lappr_information_device,  # noqa: F401
                                     montecarlo_information, mutual_information_base_scheme,
                                     mutual_information_base_scheme_arg, mutual_information_X_Xhat,
                                     mutual_information_X_Y, mutual_information_X_Y_int_arg)

__all__ = ["P_xhat", "montecarlo_information", "mutual_information_X_Xhat", "mutual_information_base_scheme",
           "mutual_information_base_scheme_arg", "mutual_information_X_Y", "mutual_information_X_Y_int_arg",
           "lappr_information", "lappr_information_device"]
