from .synthetic import SyntheticMovingMNIST  # noqa: F401
from .moving_mnist import MovingMNIST, MovingMNISTLoader, load_mnist_digits  # noqa: F401
