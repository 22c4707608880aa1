from .batched import BatchedForestFireHelicopterEnv
from .helicopter import ForestFireHelicopterEnv
from .policy import HelicopterPolicy

__all__ = ["ForestFireHelicopterEnv", "BatchedForestFireHelicopterEnv", "HelicopterPolicy"]
