"""
Pack compaction policy.

Once per-model early stopping has ended enough models of a pack, the
fit goes on in a smaller pack that holds the live models only
(``BasePack._fit_epochs``). The decision is a pure function of the
current pack's size and the number of live models:

    compact  <=>  n_live >= 1  and  n_live < ratio * G_current

With the default ratio 0.5 a pack of 2 never compacts and every
compaction at least halves the pack, so all compactions of a fit
together move less state than one extra pass over the parent's; ratio
1.0 compacts at every stop.

Environment, read when a fit with early stopping starts:

``GORDO_PACK_COMPACT``        ``0`` disables compaction.
``GORDO_PACK_COMPACT_RATIO``  float in (0, 1], default 0.5; anything
                              else raises ValueError.
"""
from __future__ import annotations

import math
import os
from typing import Optional

DEFAULT_RATIO = 0.5


def check_ratio(ratio) -> float:
    try:
        r = float(ratio)
    except (TypeError, ValueError):
        r = math.nan
    if not (0.0 < r <= 1.0):  # NaN fails both comparisons
        raise ValueError(
            f"the pack compaction ratio must be a float in (0, 1], got "
            f"{ratio!r}"
        )
    return r


def should_compact(G_current: int, n_live: int,
                   ratio: float = DEFAULT_RATIO) -> bool:
    """Whether a pack of ``G_current`` models of which ``n_live`` still
    train continues as a pack of ``n_live``."""
    r = check_ratio(ratio)
    return 1 <= int(n_live) < r * int(G_current)


def ratio_from_env() -> Optional[float]:
    """The ratio this fit compacts at; None when compaction is off."""
    ratio = check_ratio(
        os.environ.get("GORDO_PACK_COMPACT_RATIO", DEFAULT_RATIO)
    )
    if os.environ.get("GORDO_PACK_COMPACT", "1") == "0":
        return None
    return ratio
