"""Recipe and stand-in headers that compile the reference rasterizer for the CPU (test infrastructure only)."""
