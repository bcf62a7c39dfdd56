from dist_classicrl_amd.algorithms.population import PopulationRun, QLearningPopulation

__all__ = ["PopulationRun", "QLearningPopulation"]
