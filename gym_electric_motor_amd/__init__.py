"""gym_electric_motor_amd -- MI355X-native batched physical-system stepper for gym-electric-motor (GEM).

One hot path only: `SCMLSystem.simulate()` / `reset()` for N independent env instances, in hand-written HIP
kernels behind GEM's `PhysicalSystem` plugin surface (include/gemx.h).
"""
from . import _lib  # noqa: F401
from .components import (  # noqa: F401
    ConstantSpeedLoad,
    ContB6BridgeConverter,
    ContFourQuadrantConverter,
    ContMultiConverter,
    DcExternallyExcitedMotor,
    DcPermanentlyExcitedMotor,
    DcSeriesMotor,
    DcShuntMotor,
    DoublyFedInductionMotor,
    DormandPrince5Solver,
    ScipyOdeSolver,
    EulerSolver,
    ExternallyExcitedSynchronousMotor,
    FiniteB6BridgeConverter,
    FiniteFourQuadrantConverter,
    FiniteMultiConverter,
    IdealVoltageSupply,
    PermanentMagnetSynchronousMotor,
    PolynomialStaticLoad,
    RCVoltageSupply,
    RK4Solver,
    SquirrelCageInductionMotor,
    SynchronousReluctanceMotor,
)
from .envs import BatchedElectricMotorEnv, CompleteBatchedElectricMotorEnv, default_components, default_env_modules, default_ode_solver, default_physical_system_wrappers, make  # noqa: F401
from .reference_generators import BatchedWienerProcessReferenceGenerator, ReplayReferenceGenerator  # noqa: F401
from .reference_generators import ProfileReferenceGenerator, ProfileReferences  # noqa: F401
from .reference_generators import (  # noqa: F401
    BatchedMultipleReferenceGenerator, ConstReferenceGenerator, LaplaceProcessReferenceGenerator, SawtoothReferenceGenerator,
    SinusoidalReferenceGenerator, StepReferenceGenerator, SwitchedReferenceGenerator, TriangularReferenceGenerator, WienerProcessReferenceGenerator,
)
from .physical_system_wrappers import CosSinProcessor, CurrentSumProcessor, DeadTimeProcessor, DqToAbcActionProcessor, FluxObserver, FluxOrientedDqToAbcActionProcessor  # noqa: F401
from .physical_system_wrappers import StateNoiseProcessor  # noqa: F401
from .flux_observer import FluxObserverStage  # noqa: F401
from .state_noise import StateNoiseStage  # noqa: F401
from .episodes import EpisodeStage  # noqa: F401
from .env_parameters import EnvParameters  # noqa: F401
from .policy import MLPPolicy  # noqa: F401
from .returns import advantages, bind_advantages, bind_discounted_returns, discounted_returns  # noqa: F401
from .observation import ObservationStage  # noqa: F401
from .physical_systems import (  # noqa: F401
    BatchedDcMotorSystem,
    BatchedDoublyFedInductionMotorSystem,
    BatchedExternallyExcitedSynchronousMotorSystem,
    BatchedSCMLSystem,
    BatchedSquirrelCageInductionMotorSystem,
    BatchedSynchronousMotorSystem,
    LimitConstraint,
    SquaredConstraint,
)

__version__ = "0.1.0"
