"""Simulator protocol, trajectory container, neighbour helpers, the HIP MD simulator (fused Langevin kernel) and the\numbrella sampler built on it."""

from mythos_amd.simulators.umbrella import HipUmbrellaSampler, UmbrellaInfo, UmbrellaRecord  # noqa: F401
