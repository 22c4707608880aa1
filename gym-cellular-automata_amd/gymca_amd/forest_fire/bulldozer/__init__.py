from .advanced import AdvancedForestFireBulldozerEnv
from .batched import BatchedForestFireBulldozerEnv
from .bulldozer import ForestFireBulldozerEnv
from .policy import BulldozerPolicy, ExtensionBulldozerPolicy

__all__ = ["ForestFireBulldozerEnv", "BatchedForestFireBulldozerEnv", "AdvancedForestFireBulldozerEnv",
           "BulldozerPolicy", "ExtensionBulldozerPolicy"]
