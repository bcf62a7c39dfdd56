from dist_classicrl_amd.algorithms.population import (
    PopulationEval,
    PopulationRun,
    PopulationTraining,
    QLearningPopulation,
)

__all__ = ["PopulationEval", "PopulationRun", "PopulationTraining", "QLearningPopulation"]
