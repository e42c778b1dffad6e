"""graph_weather/models/fengwu_ghr of the reference (LoRAModule is not provided: see graph_weather_amd/fengwu_ghr.py)."""
