from .batched import BatchedForestFireHelicopterEnv
from .helicopter import ForestFireHelicopterEnv

__all__ = ["ForestFireHelicopterEnv", "BatchedForestFireHelicopterEnv"]
