from .comm import (  # noqa: F401
    Communicator,
    init,
    finalize,
    flush,
    get_default_comm,
    get_world,
    COMM_WORLD,
)
from .grid import CartesianGrid  # noqa: F401
from .halo import HaloExchanger  # noqa: F401
from . import halo  # noqa: F401
from .stencil import HaloStencil  # noqa: F401
from . import stencil  # noqa: F401
from .cg import CGInfo, StencilCG  # noqa: F401
from . import cg  # noqa: F401
from .chebyshev import ChebyshevInfo, StencilChebyshev  # noqa: F401
from . import chebyshev  # noqa: F401
from .ddp import average_gradients  # noqa: F401
from .tp import (  # noqa: F401
    ColumnParallelLinear,
    RowParallelLinear,
    copy_to_parallel,
)
from .sp import seq_to_head_shard, head_to_seq_shard  # noqa: F401
from .pp import (  # noqa: F401
    send_activation,
    recv_activation,
    backward_send,
)
