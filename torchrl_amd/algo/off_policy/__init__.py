from .off_rl_algo import OffRLAlgo
from .twin_sac_q import TwinSACQ
from .sac_v import SAC, TwinSAC
from .dqn import DQN, QRDQN
from .bootstrapped_dqn import BootstrappedDQN
from .det_ac import DDPG, TD3
