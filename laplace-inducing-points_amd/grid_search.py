"""The reference's ``src/grid_search.py``: :func:`grid_search_alpha` lives in ``train_alpha.py`` next to the evidence
fits; this module keeps ``from src.grid_search import grid_search_alpha`` working."""
from .train_alpha import grid_search_alpha, refinement_points  # noqa: F401
