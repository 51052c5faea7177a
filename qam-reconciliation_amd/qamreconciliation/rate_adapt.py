"""qamreconciliation.rate_adapt: rate adaptation of one mother code (puncturing, shortening, blind rounds),
which the reference does not have (qamr.rate_adapt)."""
from qamr.rate_adapt import (SHORTENED_LAPPR, RateAdaption, blind_batch, expand_host,  # noqa: F401
                             untainted_order)

__all__ = ["SHORTENED_LAPPR", "RateAdaption", "untainted_order", "expand_host", "blind_batch"]
