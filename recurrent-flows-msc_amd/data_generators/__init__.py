from .synthetic import SyntheticMovingMNIST  # noqa: F401
from .moving_mnist import MovingMNIST, MovingMNIST_synchronized, MovingMNISTLoader, load_mnist_digits  # noqa: F401
from .clips import ClipLoader, FrameStore  # noqa: F401
from .bair_push import PushDataset  # noqa: F401
from .kth import KTH, read_t7  # noqa: F401
from .clip_folder import ClipFolder  # noqa: F401
