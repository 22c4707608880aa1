from .advanced import AdvancedForestFireBulldozerEnv
from .batched import BatchedForestFireBulldozerEnv
from .bulldozer import ForestFireBulldozerEnv
from .policy import BulldozerPolicy

__all__ = ["ForestFireBulldozerEnv", "BatchedForestFireBulldozerEnv", "AdvancedForestFireBulldozerEnv",
           "BulldozerPolicy"]
